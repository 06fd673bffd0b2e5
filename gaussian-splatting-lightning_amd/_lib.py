"""
_lib.py — ctypes binding of libgspl_hip.so (the C-ABI declared in include/gspl_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every compute call goes
through the C-ABI with raw device pointers.  There is NO fallback: if the library is missing, or
a tensor is not on the GPU, the call raises.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from ctypes import c_float, c_int, c_void_p

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSPL_HIP_LIB", os.path.join(_PKG_DIR, "libgspl_hip.so"))   # override: A/B builds of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "gspl_hip.h")         # the in-tree header, also for an overridden library


class HipLibraryError(RuntimeError):
    pass


# The binding is READ from the header when this module is imported: entry points, constants and structs are written down once, in
# include/gspl_hip.h.  The parser knows exactly the C the header uses; whatever it cannot classify raises.
_SCALARS = {"int": c_int, "float": c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16, "int8_t": ctypes.c_int8}
_RETURNS = {"int": c_int, "size_t": ctypes.c_size_t, "void*": c_void_p, "const char*": ctypes.c_char_p}
_DECLARATION = re.compile(r"(?:const\s+)?(\w+)(\s+|\s*(?:\*\s*(?:const\b\s*)?)+)(\w+)")


def _unparsed(what, why="cannot classify"):
    raise HipLibraryError(f"gspl_hip.h: {why} `{' '.join(what.split())}`")


def _ctype(decl, types, where):
    """`[const] type[*...] name` -> (ctypes type, name); `types`: the structs and function-pointer typedefs declared so far."""
    m = _DECLARATION.fullmatch(decl.strip())
    if not m:
        _unparsed(decl, f"{where}: cannot parse the declaration")
    base, stars, name = m[1], m[2].count("*"), m[3]
    known = types.get(base, _SCALARS.get(base))
    if stars == 0 and known is not None:
        return known, name
    if stars == 1 and isinstance(known, type) and issubclass(known, ctypes.Structure):
        return ctypes.POINTER(known), name      # (the wrong struct raises; an array of the struct is accepted)
    if stars and (base == "void" or base in _SCALARS):
        return c_void_p, name
    _unparsed(decl, f"{where}: unknown type in")


def _restype(text):
    key = re.sub(r"\s*\*", "*", " ".join(text.split()))
    return _RETURNS[key] if key in _RETURNS else _unparsed(text, "unknown return type")


def _parameters(text, types, where):
    return [] if text.strip() in ("", "void") else [_ctype(p, types, where) for p in text.split(",")]


def _parse_header(text):
    """-> (constants {name: int}, types {C name: Structure subclass | CFUNCTYPE}, functions {name: (restype, argtypes, parameter names)})."""
    constants, types, functions, lines = {}, {}, {}, []
    for line in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).splitlines():
        define = re.fullmatch(r"\s*#\s*define\s+(\w+)\s*(.*?)\s*", line)
        if define and define[2]:
            constants[define[1]] = int(define[2]) if re.fullmatch(r"-?\d+", define[2]) else _unparsed(line)
        elif not line.lstrip().startswith("#"):
            lines.append(line)
        elif not define and not re.match(r"\s*#\s*(include|ifdef|ifndef|endif)\b", line):
            _unparsed(line)

    def function_pointer(m):
        types[m[2]] = ctypes.CFUNCTYPE(_restype(m[1]), *[t for t, _ in _parameters(m[3], types, m[2])])
        return ""

    def struct(m):
        fields = []
        for statement in filter(str.strip, m[2].split(";")):      # `int N, width, height`, `float* a`, `gspl_x means, scales`
            first, *more = statement.split(",")
            ctype, name = _ctype(first, types, m[1])
            if m[1] != m[3] or (more and "*" in statement) or not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
                _unparsed(statement, f"{m[1]}: cannot parse the field(s)")
            fields += [(n.strip(), ctype) for n in [name] + more]
        python_name = "".join(word.capitalize() for word in m[1][len("gspl_"):].split("_"))
        types[m[1]] = type(python_name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"`{m[1]}` of include/gspl_hip.h."})
        return ""

    def enum(m):
        for item in m[1].split(","):
            entry = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item) or _unparsed(item, "cannot parse the enumerator")
            constants[entry[1]] = int(entry[2])
        return ""

    text = "\n".join(lines)
    text = re.sub(r"typedef\s+([\w\s*]+?)\(\s*\*\s*(\w+)\s*\)\s*\(([^()]*)\)\s*;", function_pointer, text)
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"enum\s*\{([^{}]*)\}\s*;", enum, text)
    *prototypes, rest = re.sub(r'extern\s+"C"\s*\{', "", text).split(";")
    if rest.strip() not in ("", "}"):
        _unparsed(rest)
    for prototype in prototypes:
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(gspl_\w+)\s*\(([^()]*)\)\s*", prototype) or _unparsed(prototype)
        args = _parameters(m[3], types, m[2])
        functions[m[2]] = (_restype(m[1]), [t for t, _ in args], tuple(n for _, n in args))
    return constants, types, functions


def _read_header(path):
    try:
        with open(path) as f:
            return _parse_header(f.read())
    except OSError as e:
        raise HipLibraryError(f"{path} not readable ({e}): the ctypes binding of this package is read from it; there is no other table") from e


_CONSTANTS, _TYPES, _FUNCTIONS = _read_header(HEADER_PATH)
globals().update({name: value for name, value in _CONSTANTS.items() if name.startswith("GSPL_")})      # every GSPL_* of the header
ABI_VERSION = _CONSTANTS["GSPL_ABI_VERSION"]
CAMERA_MODELS = {"pinhole": _CONSTANTS["GSPL_CAMERA_PINHOLE"], "ortho": _CONSTANTS["GSPL_CAMERA_ORTHO"], "fisheye": _CONSTANTS["GSPL_CAMERA_FISHEYE"]}
ALLOC_FN = _TYPES["gspl_alloc_fn"]
AdamTensor, BwdAdamTensor, BwdAdamPlan, InriaState, SurfelState = (
    _TYPES[name] for name in ("gspl_adam_tensor", "gspl_bwd_adam_tensor", "gspl_bwd_adam_plan", "gspl_inria_state", "gspl_surfel_state"))
_SIGNATURES = {name: (restype, argtypes) for name, (restype, argtypes, _) in _FUNCTIONS.items()}

_LIB = None


def exported_symbols():
    """Names include/gspl_hip.h declares (used by the no-GPU ABI test)."""
    return sorted(_SIGNATURES)


def build(verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_PKG_DIR, "csrc"), "-j8"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise HipLibraryError("building libgspl_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """Load libgspl_hip.so (once).  Raises HipLibraryError when it is absent — there is no CPU path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: the HIP extension is the only compute path of this package. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
            f"{os.path.join(_PKG_DIR, 'csrc')}`.")
    try:
        handle = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"could not load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in _SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    got = handle.gspl_abi_version()
    if got != ABI_VERSION:
        raise HipLibraryError(f"ABI mismatch: library {got}, python binding {ABI_VERSION}; rebuild the extension")
    if handle.gspl_inria_state_bytes() != ctypes.sizeof(InriaState):
        raise HipLibraryError(f"gspl_inria_state: the library's struct has {handle.gspl_inria_state_bytes()} bytes, the binding's "
                              f"{ctypes.sizeof(InriaState)}; rebuild the extension")
    if handle.gspl_surfel_state_bytes() != ctypes.sizeof(SurfelState):
        raise HipLibraryError(f"gspl_surfel_state: the library's struct has {handle.gspl_surfel_state_bytes()} bytes, the binding's "
                              f"{ctypes.sizeof(SurfelState)}; rebuild the extension")
    _LIB = handle
    return _LIB


# Optional per-call device timing (bench.py): a list that receives (name, start_event, end_event).
# Events are recorded on torch's current stream, which is the stream every kernel is launched on.
_PROFILE = None
_PROFILE_PERIOD = 1
_PROFILE_SEEN: dict = {}
_PROFILE_NAMES = None


def profile_start(names=None, period: int = 1):
    """Time C-ABI calls with events on the current stream; `names`: only these entry points (None: all); `period`: every
    period-th call of a name is timed (an event pair costs the stream ~6 us of idle time on either side of the call)."""
    global _PROFILE, _PROFILE_NAMES, _PROFILE_PERIOD, _PROFILE_SEEN
    _PROFILE = []
    _PROFILE_NAMES = None if names is None else frozenset(names)
    _PROFILE_PERIOD, _PROFILE_SEEN = max(int(period), 1), {}
    on = lambda name: _PROFILE_PERIOD if (_PROFILE_NAMES is None or name in _PROFILE_NAMES) else 0
    lib().gspl_profile_enable2(on("gspl_composite_fwd"), on("gspl_composite_bwd_packed"))


def profile_stop():
    """Returns {name: [ms, ...]} (synchronises).  The compositing launches made inside the fused Inria calls are reported
    under the names of their stage entry points (as one entry holding the mean, repeated per launch)."""
    global _PROFILE
    rec, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in rec or []:
        out.setdefault(name, []).append(e0.elapsed_time(e1))
    for which, name in ((0, "gspl_composite_fwd"), (1, "gspl_composite_bwd_packed")):
        n, ms = c_int(0), c_float(0.0)
        check(lib().gspl_profile_read(which, ctypes.byref(n), ctypes.byref(ms)), "gspl_profile_read")
        if n.value > 0 and (_PROFILE_NAMES is None or name in _PROFILE_NAMES):
            out.setdefault(name, []).extend([ms.value / n.value] * n.value)
    lib().gspl_profile_enable(0)
    return out


def call(name: str, *args):
    """Invoke one C-ABI entry point and raise on a non-zero status."""
    fn = getattr(lib(), name)
    timed = _PROFILE is not None and (_PROFILE_NAMES is None or name in _PROFILE_NAMES)
    if timed and _PROFILE_PERIOD > 1:
        seen = _PROFILE_SEEN.get(name, 0)
        _PROFILE_SEEN[name] = seen + 1
        timed = seen % _PROFILE_PERIOD == 0
    try:
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            _PROFILE.append((name, e0, e1))
        else:
            rc = fn(*args)
    except ctypes.ArgumentError as e:      # "argument 17: TypeError: ..." -> "gspl_x: argument 17 (v_rows): ..."
        names = _FUNCTIONS[name][2]
        named = re.sub(r"argument (\d+)", lambda m: f"argument {m[1]} ({names[int(m[1]) - 1]})" if int(m[1]) <= len(names) else m[0], str(e), count=1)
        raise ctypes.ArgumentError(f"{name}: {named}") from e
    check(rc, name)


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().gspl_last_error()
        raise RuntimeError(f"{what} failed (status {rc}): {msg.decode() if msg else '?'}")


def ptr(t, dtype=None, offset_bytes: int = 0):
    """Device pointer of a contiguous CUDA/HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("gspl ops run on the GPU only (tensor is on %s); there is no CPU fallback" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("gspl ops need contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    return c_void_p(t.data_ptr() + offset_bytes)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


class device_guard:
    """`with device_guard(tensor):` makes the tensor's device current for the enclosed launches (so that `stream()` hands
    out THAT device's current stream) and restores the previous one; free when it already is the current device."""
    __slots__ = ("idx", "prev")

    def __init__(self, t):
        dev = t.device if hasattr(t, "device") else t
        self.idx = dev.index if dev.index is not None else (_raw_device() if _raw_device is not None else torch.cuda.current_device())
        self.prev = -1

    def __enter__(self):
        cur = _raw_device() if _raw_device is not None else torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def stream():
    """Raw handle of torch's current stream on the current device.  `torch.cuda.current_stream().cuda_stream` costs ~10 us
    of Python per call (device-index plumbing, a Stream object) and every op wrapper needs it: the C accessors do the
    same in well under a microsecond."""
    if _raw_stream is not None and _raw_device is not None:
        return c_void_p(_raw_stream(_raw_device()))
    return c_void_p(torch.cuda.current_stream().cuda_stream)

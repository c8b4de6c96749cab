"""ctypes binding of liblwsnet_hip.so.  include/lwsnet_hip.h is the statement of the C ABI: PROTOTYPES and the LWS_*
constants are read from it when this module is imported (tests/test_abi_cpu.py has a C++ compiler check the reading).  The entry
points added behind ABI v8 live in headers of their own, named in HEADERS; each is read the same way into ABI[header name], and a
new header is one more name there.  HEADERS, ABI and ALL_PROTOTYPES are the functions the stream-ordering table of
tests/test_gpu_stream_order.py has a row for; lws_tsdf_mesh's header and lws_track's (include/lwsnet_track.h) are read the same way
into tables of their own beside these, MESH_ABI and TRACK_ABI, as is lws_tsdf_window's (include/lwsnet_tsdf_window.h) into WINDOW_ABI
and lws_movers' (include/lwsnet_movers.h) into MOVERS_ABI, and their calls' stream tests are in their own test files.

The header cannot say which pointers are host pointers, so every pointer but `const char *` is c_void_p: the 20 host-pointer
parameters -- lws_set_tensor's data and shape, the mean / std arrays, lws_profile_read*, lws_clock_read, lws_join_stats, the
handle out-parameters and lws_create's config -- carry no POINTER(...) type.  ctypes converts byref(x), arrays and typed pointer
objects to c_void_p parameters, so callers pass what they always passed.

There is no CPU fallback: if the library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblwsnet_hip.so")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HEADERS = ("lwsnet_hip.h", "lwsnet_objects.h", "lwsnet_temporal.h", "lwsnet_egomotion.h", "lwsnet_tsdf.h")      # the base header first
MESH_HEADERS = ("lwsnet_tsdf_mesh.h",)
TRACK_HEADERS = ("lwsnet_track.h",)
WINDOW_HEADERS = ("lwsnet_tsdf_window.h",)
MOVERS_HEADERS = ("lwsnet_movers.h",)
HEADER_PATH = os.path.join(INCLUDE, HEADERS[0])

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int64_p = ctypes.POINTER(ctypes.c_int64)


class LwsConfig(ctypes.Structure):
    _fields_ = [("maxdisplist", ctypes.c_int32 * 3), ("layers_3d", ctypes.c_int32),
                ("channels_3d", ctypes.c_int32), ("growth_rate", ctypes.c_int32 * 3),
                ("feature_fp16", ctypes.c_int32), ("interp_align_mode", ctypes.c_int32)]


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double}
_HANDLES = ("lws_handle", "lws_pool_handle")


def _ctype(decl, named):
    """One parameter (`named`) or return type as written in C -> (ctypes type, the C spelling without the name, such as
    `const float *` or `float *const [4]`).  What the rules of parse_header do not cover raises ValueError."""
    m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?" if named else r"(.*)()()", decl.strip(), re.S)      # type, name, [N]
    tokens = re.findall(r"\w+|\*|\S", m[1]) if m else []
    base = [t for t in tokens if t not in ("const", "*")]
    if len(base) != 1 or not re.fullmatch(r"\w+", base[0]):
        raise ValueError(f"cannot read `{' '.join(decl.split())}` as a type{' and a name' if named else ''}")
    base, stars, n = base[0], tokens.count("*"), m[3]
    spelling = " ".join(tokens).replace("* ", "*") + (f" [{n}]" if n else "")
    if stars > 1:
        raise ValueError(f"`{spelling}` is a pointer to a pointer")
    if n:
        if not stars:
            raise ValueError(f"`{spelling}` is an array of non-pointers")
        return ctypes.c_void_p * int(n), spelling
    if stars:
        return (ctypes.c_char_p if tokens[:2] == ["const", "char"] else ctypes.c_void_p), spelling
    if base in _HANDLES:
        return ctypes.c_void_p, spelling
    if base not in _SCALARS:
        raise ValueError(f"unknown type name `{base}`")
    return _SCALARS[base], spelling


def parse_header(text, where="header"):
    """Reads a C header written like include/lwsnet_hip.h.  Returns (prototypes, spellings, constants):
    prototypes {function: (restype, [argtypes])}, spellings {function: (return type, [parameter types])} as C text, constants
    {name: int} from `#define NAME <integer>` and enum entries `NAME = <integer>`.  Scalars map by name (int, int32_t, int64_t,
    uint32_t, float, double); lws_handle, lws_pool_handle and every pointer map to c_void_p, except `const char *`: c_char_p;
    `T *name[N]` and `T *const name[N]` map to c_void_p * N.  Anything else -- an unknown type name, an array of non-pointers,
    a pointer to a pointer -- raises ValueError naming the function and the parameter: nothing defaults to int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{(.*?)\}", text, re.S):
        for entry in filter(None, (e.strip() for e in body.split(","))):
            m = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", entry)
            if not m:
                raise ValueError(f"{where}: enum entry `{entry}` has no integer value written out")
            consts[m[1]] = int(m[2])
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)                   # preprocessor lines
    text = re.sub(r"extern\s*\"C\"\s*\{|\{[^{}]*\}|\}", " ", text)             # the extern "C" braces, struct and enum bodies
    protos, spellings = {}, {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        if stmt.startswith("typedef"):
            continue
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, re.S)
        if not m:
            raise ValueError(f"{where}: cannot read `{' '.join(stmt.split())}` as a function declaration")
        name, params = m[2], [] if m[3].strip() == "void" else m[3].split(",")
        try:
            res = _ctype(m[1], False)
        except ValueError as e:
            raise ValueError(f"{where}: {name}: return type: {e}") from None
        args = []
        for i, p in enumerate(params):
            try:
                args.append(_ctype(p, True))
            except ValueError as e:
                pname = re.findall(r"[A-Za-z_]\w*", p)[-1:] or [f"#{i + 1}"]
                raise ValueError(f"{where}: {name}: parameter `{pname[0]}`: {e}") from None
        protos[name] = (res[0], [a[0] for a in args])
        spellings[name] = (res[1], [a[1] for a in args])
    return protos, spellings, consts


def merge_headers(tables):
    """{header name: prototypes} -> the one table load() binds, {function: (restype, argtypes)}; a function that two headers
    declare raises ValueError naming it and both headers."""
    merged, origin = {}, {}
    for header, protos in tables.items():
        for name in protos:
            if name in origin:
                raise ValueError(f"{name} is declared by {origin[name]} and by {header}")
            origin[name] = header
        merged.update(protos)
    return merged


def _read(name):
    """include/<name> -> ((prototypes, spellings, path), constants)"""
    with open(os.path.join(INCLUDE, name)) as f:
        protos, spellings, consts = parse_header(f.read(), f.name)
    return (protos, spellings, f.name), consts


_READ = {name: _read(name) for name in (*HEADERS, *MESH_HEADERS, *TRACK_HEADERS, *WINDOW_HEADERS, *MOVERS_HEADERS)}
# header name -> (prototypes, spellings, path): name -> (restype, argtypes) and name -> (C return type, C parameter types), exactly
# the functions that header declares; PROTOTYPES, C_SPELLINGS and the constants are the base header's
ABI = {name: _READ[name][0] for name in HEADERS}
_CONSTANTS = _READ[HEADERS[0]][1]
PROTOTYPES, C_SPELLINGS = ABI[HEADERS[0]][:2]
(LWS_ABI_VERSION, LWS_OK, LWS_ERR_INVALID, LWS_ERR_HIP, LWS_ERR_STATE, LWS_ERR_NOMEM, LWS_KC_COUNT, LWS_SPARS_BINS,
 LWS_POOL_SIDE_STREAMS) = (_CONSTANTS[k] for k in ("LWS_ABI_VERSION", "LWS_OK", "LWS_ERR_INVALID", "LWS_ERR_HIP", "LWS_ERR_STATE",
                                                   "LWS_ERR_NOMEM", "LWS_KC_COUNT", "LWS_SPARS_BINS", "LWS_POOL_SIDE_STREAMS"))
LWS_DELAY_F4, LWS_DELAY_F2, LWS_DELAY_LEFT, LWS_DELAY_CHUNKS, LWS_DELAY_ALL = (
    _CONSTANTS[k] for k in ("LWS_DELAY_F4", "LWS_DELAY_F2", "LWS_DELAY_LEFT", "LWS_DELAY_CHUNKS", "LWS_DELAY_ALL"))      # lws_debug_delay_side
ALL_PROTOTYPES = merge_headers({name: table[0] for name, table in ABI.items()})
# lws_tsdf_mesh: the same three per header, and what load() binds of it
MESH_ABI = {name: _READ[name][0] for name in MESH_HEADERS}
LWS_TSDF_MESH_MAX_TRIS = _READ[MESH_HEADERS[0]][1]["LWS_TSDF_MESH_MAX_TRIS"]
MESH_PROTOTYPES = merge_headers({name: table[0] for name, table in MESH_ABI.items()})
# lws_track and lws_track_normal: likewise
TRACK_ABI = {name: _READ[name][0] for name in TRACK_HEADERS}
TRACK_PROTOTYPES = merge_headers({name: table[0] for name, table in TRACK_ABI.items()})
# lws_tsdf_window: likewise
WINDOW_ABI = {name: _READ[name][0] for name in WINDOW_HEADERS}
WINDOW_PROTOTYPES = merge_headers({name: table[0] for name, table in WINDOW_ABI.items()})
# lws_movers: likewise
MOVERS_ABI = {name: _READ[name][0] for name in MOVERS_HEADERS}
MOVERS_PROTOTYPES = merge_headers({name: table[0] for name, table in MOVERS_ABI.items()})
merge_headers({name: table[0] for name, table in (*ABI.items(), *MESH_ABI.items(), *TRACK_ABI.items(), *WINDOW_ABI.items(), *MOVERS_ABI.items())})       # a name two headers declare raises

_lib = None


def load():
    """Loads the library (building is the job of __graft_entry__.build / lwsnet_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP/HSA runtime (torch/lib/libamdhip64.so).  It must be the first HIP runtime in
    # the process: loading this library first pulls /opt/rocm's copy in, and the second runtime then reports "no
    # ROCm-capable device".  With torch imported first, the SONAME libamdhip64.so.7 resolves to torch's copy and both
    # share one runtime (device pointers and streams interoperate).
    import torch  # noqa: F401
    from . import late_env
    if late_env():
        import warnings
        warnings.warn(f"lwsnet_amd was imported after HIP had initialised in this process: {', '.join(late_env())} could not be "
                      "exported in time (import lwsnet_amd before the first torch.cuda call, or export them in the environment); "
                      "multi-stream forwards / RCCL may run slower or fail (lwsnet_amd/__init__.py)", RuntimeWarning, stacklevel=2)
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -m lwsnet_amd.build`); there is no CPU fallback for the disparity path")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (*ALL_PROTOTYPES.items(), *MESH_PROTOTYPES.items(), *TRACK_PROTOTYPES.items(), *WINDOW_PROTOTYPES.items(),
                              *MOVERS_PROTOTYPES.items()):
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.lws_abi_version() != LWS_ABI_VERSION:
        raise RuntimeError("liblwsnet_hip.so ABI version mismatch; rebuild the extension")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc == LWS_OK:
        return
    msg = load().lws_last_error().decode("utf-8", "replace")
    if rc == LWS_ERR_INVALID:
        raise ValueError(msg or what)
    raise RuntimeError(f"{what}: {msg} (status {rc})")


def call(name, *args):
    """The library's function `name` on args; a status other than LWS_OK raises (check).  The one place a name is given."""
    check(getattr(load(), name)(*args), name)


def nbytes(name, *dims):
    """What a *_workspace function answers for dims: a byte count; a negative answer is a status and raises (check)."""
    n = getattr(load(), name)(*dims)
    if n < 0:
        check(n, name)
    return n

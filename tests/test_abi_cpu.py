"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol
include/lwsnet_hip.h declares; host-side argument / state errors behave like the
reference's Python exceptions (ValueError for bad shapes, RuntimeError otherwise).
lwsnet_amd._lib reads its prototypes and constants from that header: its reading is held to a C++ compiler, to hand-written
expectations and, on small header texts, to every rule it states."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lwsnet_amd import _lib
from lwsnet_amd.weights import default_args, make_state_dict


def _declared():
    txt = open(os.path.join(ROOT, "include", "lwsnet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lws_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_prototypes_agree():
    assert _declared() == sorted(_lib.PROTOTYPES)


# ---- the reader of include/lwsnet_hip.h (lwsnet_amd._lib.parse_header) ----
VP, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def _host_compiler():
    """g++, or the clang++ of the toolchain hipcc belongs to; a box that builds the library has one of them."""
    from lwsnet_amd import build
    cands = [shutil.which("g++"), shutil.which("clang++")]
    try:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
        cands += [os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")]
    except RuntimeError:
        pass
    found = [c for c in cands if c and os.path.isfile(c)]
    assert found, f"no host C++ compiler among {cands}: the reading of the header cannot be checked"
    return found[0]


def _assert_line(name, spelling):
    ret, params = spelling
    return f'static_assert(std::is_same_v<decltype(&{name}), {ret} (*)({", ".join(params)})>, "{name}");\n'


def compiles(header, path, lines):
    """The host compiler's run over `lines` behind an include of `header`, syntax only."""
    with open(path, "w") as f:
        f.write(f'#include <cstddef>\n#include <type_traits>\n#include "{header}"\n' + "".join(lines))
    return subprocess.run([_host_compiler(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(path)], capture_output=True, text=True)


def test_a_compiler_agrees_with_the_reading(tmp_path):
    """Per declared function, the parameter and return types the reader kept, as C text, are the function's type to a C++
    compiler; one scalar misread fails the compile and names the function; LwsConfig has lws_config's size and offsets."""
    assert sorted(_lib.C_SPELLINGS) == _declared() and len(_lib.C_SPELLINGS) == 67
    lines = {name: _assert_line(name, sp) for name, sp in _lib.C_SPELLINGS.items()}
    config = [f'static_assert(sizeof(lws_config) == {ctypes.sizeof(_lib.LwsConfig)}, "sizeof(lws_config)");\n']
    for field, _ in _lib.LwsConfig._fields_:
        d = getattr(_lib.LwsConfig, field)
        config.append(f'static_assert(offsetof(lws_config, {field}) == {d.offset} && sizeof(lws_config::{field}) == {d.size}, "{field}");\n')
    assert len(config) == 7
    ok = compiles("lwsnet_hip.h", tmp_path / "abi.cpp", list(lines.values()) + config)
    assert ok.returncode == 0, ok.stderr
    # lws_softargmin(const float *, float *, int, int, int, int, float, void *): its fourth int read as float
    ret, params = _lib.C_SPELLINGS["lws_softargmin"]
    assert params[5] == "int" and params[6] == "float"
    flipped = dict(lines, lws_softargmin=_assert_line("lws_softargmin", (ret, params[:5] + ["float"] + params[6:])))
    bad = compiles("lwsnet_hip.h", tmp_path / "abi_flipped.cpp", list(flipped.values()) + config)
    assert bad.returncode != 0 and '"lws_softargmin"' in bad.stderr, bad.stderr
    assert bad.stderr.count("error:") == 1, bad.stderr
    # ... and a field of the structure moved by four bytes
    moved = compiles("lwsnet_hip.h", tmp_path / "abi_moved.cpp", [config[2].replace("== 12 ", "== 16 ")])
    assert "== 16 " in config[2].replace("== 12 ", "== 16 ") and moved.returncode != 0 and "layers_3d" in moved.stderr, moved.stderr


# written by hand from the header, not from the reader: every parameter kind, the two longest lists, the three return types
EXPECTED = {
    "lws_ground_fit": (I, [VP, VP, VP, I, I, I, F, I, I, I, I, I, I, I, I, F, F, I, VP, VP, VP, VP]),
    "lws_stixels": (I, [VP, VP, VP, VP, I, I, I, F, F, I, I, I, I, I, I, I, I, I, VP, VP, VP, VP]),
    "lws_rectify_pair": (I, [VP * 2, VP, I, I, I, I, I, I, I, I, VP, VP, VP * 2, VP * 2, VP * 2, VP * 2, VP]),
    "lws_photometric": (I, [VP * 4, I, VP, VP, VP * 4, VP, I, I, I, F, VP * 4, VP * 4, VP * 4, VP, VP]),
    "lws_softargmin_conf": (I, [VP, I, I, I, I, F, I, I, VP, VP, VP, VP, VP, VP]),
    "lws_stage_metrics_workspace": (ctypes.c_int64, [I, I, I]),
    "lws_pool_submit": (I, [VP, VP, VP, I, I, I, VP * 4, VP, VP]),
    "lws_last_error": (ctypes.c_char_p, []),
    # the scalar kinds the eight above do not hold: int64_t and uint32_t by value, const char * as a parameter
    "lws_apply_lut8": (I, [VP, VP, VP, ctypes.c_int64, VP]),
    "lws_debug_fill_workspace": (I, [VP, ctypes.c_uint32, VP]),
    "lws_set_tensor": (I, [VP, ctypes.c_char_p, VP, VP, I]),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_prototypes_against_hand_written_expectations(name):
    assert _lib.PROTOTYPES[name] == EXPECTED[name]
    assert len(EXPECTED["lws_ground_fit"][1]) == len(EXPECTED["lws_stixels"][1]) == 22 == max(len(a) for _, a in _lib.PROTOTYPES.values())


def test_constants_come_from_the_header():
    assert _lib.LWS_ABI_VERSION == 8 and _lib.LWS_KC_COUNT == 14 and _lib.LWS_SPARS_BINS == 1026 and _lib.LWS_POOL_SIDE_STREAMS == 1
    assert (_lib.LWS_OK, _lib.LWS_ERR_INVALID, _lib.LWS_ERR_HIP, _lib.LWS_ERR_STATE, _lib.LWS_ERR_NOMEM) == (0, -1, -2, -3, -4)
    assert _lib.c_float_p is ctypes.POINTER(ctypes.c_float) and _lib.c_int64_p is ctypes.POINTER(ctypes.c_int64)


# ---- the headers behind include/lwsnet_hip.h (lwsnet_amd._lib.ABI) ----
I64 = ctypes.c_int64
# written by hand from each header, not from the reader.  source: the file of lwsnet_amd.build.SOURCES that defines its functions;
# protos: every function's (restype, argtypes); lengths: the long parameter lists, counted; spelled: (function, position) -> the C
# text of that parameter; flip: the (function, position) of an int that a compiler must refuse to take for a float
EXTENSIONS = {
    "lwsnet_objects.h": dict(
        source="lws_objects.hip",
        protos={"lws_objects": (I, [VP, VP, VP, VP, I, I, I, F, F, I, I, I, I, I, I, I, VP, VP, VP, VP, VP, VP]),
                "lws_objects_workspace": (I64, [I, I, I, I])},
        lengths={"lws_objects": 22}, flip=("lws_objects", 6), spelled={("lws_objects", 6): "int", ("lws_objects", 7): "float"}),
    "lwsnet_temporal.h": dict(
        source="lws_temporal.hip",
        protos={"lws_temporal_step": (I, [VP] * 8 + [I, I, I] + [F] * 6 + [I, F, F] + [VP] * 7), "lws_temporal_workspace": (I64, [I, I, I, I])},
        lengths={"lws_temporal_step": 27}, flip=("lws_temporal_step", 17),
        spelled={("lws_temporal_step", 16): "float", ("lws_temporal_step", 17): "int", ("lws_temporal_step", 18): "float"}),      # max_jump, hold, q_hold
    "lwsnet_egomotion.h": dict(
        source="lws_egomotion.hip",
        protos={"lws_ego_normal": (I, [VP] * 6 + [I, I, I, I, F, F] + [VP] * 4), "lws_egomotion": (I, [VP] * 6 + [I] * 5 + [F] * 4 + [I] + [VP] * 7),
                "lws_egomotion_workspace": (I64, [I, I, I, I])},
        lengths={"lws_egomotion": 23, "lws_ego_normal": 16}, flip=("lws_egomotion", 15),
        spelled={("lws_egomotion", 14): "float", ("lws_egomotion", 15): "int", ("lws_egomotion", 16): "void *",                 # damping, min_pixels, workspace
                 ("lws_ego_normal", 5): "const double *"}),
    "lwsnet_tsdf.h": dict(
        source="lws_tsdf.hip",
        protos={"lws_tsdf_integrate": (I, [VP] * 7 + [I] * 3 + [VP] * 3 + [I] * 3 + [F] * 10 + [I, F, VP, VP]),
                "lws_tsdf_raycast": (I, [VP, VP] + [I] * 3 + [F] * 4 + [VP, VP] + [I] * 3 + [F, F, I, F] + [VP] * 4),
                "lws_tsdf_points": (I, [VP] * 3 + [I] * 3 + [F] * 5 + [I64] + [VP] * 5), "lws_tsdf_points_workspace": (I64, [I, I])},
        lengths={}, flip=("lws_tsdf_integrate", 26),
        spelled={("lws_tsdf_integrate", 26): "int", ("lws_tsdf_integrate", 27): "float", ("lws_tsdf_integrate", 28): "int64_t *",  # wmode, w_max, updated
                 ("lws_tsdf_points", 11): "int64_t"}),
}


def test_every_header_is_in_the_table_and_none_declares_what_another_does():
    assert _lib.HEADERS == ("lwsnet_hip.h", *EXTENSIONS) == tuple(_lib.ABI) and _lib.ABI["lwsnet_hip.h"][0] is _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES) == 67 and _lib.ABI["lwsnet_hip.h"][1] is _lib.C_SPELLINGS
    assert len(_lib.ALL_PROTOTYPES) == sum(len(protos) for protos, _, _ in _lib.ABI.values()) == 67 + sum(len(e["protos"]) for e in EXTENSIONS.values())


def test_a_function_declared_by_two_headers_is_refused():
    one = _lib.parse_header("int lws_a(int B);\nint lws_twice(const float *x, void *stream);\n", "one.h")[0]
    two = _lib.parse_header("int64_t lws_twice(int B);\nint lws_b(void);\n", "two.h")[0]
    assert list(_lib.merge_headers({"one.h": one, "other.h": {"lws_b": two["lws_b"]}})) == ["lws_a", "lws_twice", "lws_b"]
    with pytest.raises(ValueError, match=r"^lws_twice is declared by one\.h and by two\.h$"):
        _lib.merge_headers({"one.h": one, "two.h": two})


@pytest.mark.parametrize("header", sorted(EXTENSIONS))
def test_prototypes_of_an_extension_header(header, hip_lib):
    """The entry points of a header behind include/lwsnet_hip.h, which lwsnet_amd._lib reads into ABI[header]: exactly its functions,
    each as written by hand, bound that way on the loaded library; the table of include/lwsnet_hip.h is what it was."""
    want = EXTENSIONS[header]
    protos, spellings, path = _lib.ABI[header]
    assert sorted(protos) == sorted(spellings) == sorted(want["protos"])
    assert os.path.samefile(path, os.path.join(ROOT, "include", header))
    for name, (res, args) in want["protos"].items():
        fn = getattr(hip_lib, name)
        assert protos[name] == (res, args) and fn.argtypes == args and fn.restype is res, name
    for name, n in want["lengths"].items():
        assert len(protos[name][1]) == n, name
    assert hip_lib.lws_abi_version() == 8
    from lwsnet_amd import build
    assert want["source"] in build.SOURCES


@pytest.mark.parametrize("header", sorted(EXTENSIONS))
def test_a_compiler_agrees_with_the_reading_of_an_extension_header(header, tmp_path):
    """As above for include/lwsnet_hip.h: per function of the header, the types the reader kept, as C text, are the function's type
    to a C++ compiler; one int read as float fails the compile and names the function."""
    want, spellings = EXTENSIONS[header], _lib.ABI[header][1]
    lines = {name: _assert_line(name, sp) for name, sp in spellings.items()}
    ok = compiles(header, tmp_path / "ext.cpp", lines.values())
    assert ok.returncode == 0, ok.stderr
    for (name, k), text in want["spelled"].items():
        assert spellings[name][1][k] == text, (name, k)
    name, k = want["flip"]
    ret, params = spellings[name]
    assert params[k] == "int"
    flipped = dict(lines, **{name: _assert_line(name, (ret, params[:k] + ["float"] + params[k + 1:]))})
    bad = compiles(header, tmp_path / "ext_flipped.cpp", flipped.values())
    assert bad.returncode != 0 and f'"{name}"' in bad.stderr and bad.stderr.count("error:") == 1, bad.stderr


SMALL_HEADER = """
/* a comment that looks like a call: lws_x(left, right -> out) */
#ifndef SMALL_H
#define SMALL_H
#ifdef __cplusplus
extern "C" {
#endif
#define LWS_ANSWER 42
#define LWS_NEGATIVE -7
typedef enum { LWS_A = 0,   /* lws_y( */
               LWS_B = -3 } lws_letters;
typedef struct { int32_t v[3]; /* lws_z(int) */ } lws_thing;
typedef struct lws_ctx *lws_handle;      // lws_w(void)
typedef struct lws_pool *lws_pool_handle;
int lws_none(void);
const char *lws_text(int which, const char *key);
int64_t lws_scalars(int a, int32_t b, int64_t c, uint32_t d, float e, double f);
int lws_handles(lws_handle h, lws_pool_handle p, lws_handle *out, lws_pool_handle *pool_out);
int lws_pointers(const float *in, float *out, const uint8_t *bytes, uint16_t *words, const lws_thing *cfg, double *ms, void *stream);
int lws_arrays(const float *const maps[4], float *const out[3], uint8_t *raw[2]);
int lws_three_lines(const float *disp,   // the map
                    int B, int H,
                    int W, void *stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_maps_every_kind_of_parameter():
    protos, spellings, consts = _lib.parse_header(SMALL_HEADER)
    assert consts == {"LWS_ANSWER": 42, "LWS_NEGATIVE": -7, "LWS_A": 0, "LWS_B": -3}
    assert list(protos) == ["lws_none", "lws_text", "lws_scalars", "lws_handles", "lws_pointers", "lws_arrays", "lws_three_lines"]
    assert protos["lws_none"] == (I, []) and spellings["lws_none"] == ("int", [])
    assert protos["lws_text"] == (ctypes.c_char_p, [I, ctypes.c_char_p]) and spellings["lws_text"] == ("const char *", ["int", "const char *"])
    assert protos["lws_scalars"] == (ctypes.c_int64, [I, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, F, ctypes.c_double])
    assert protos["lws_handles"] == (I, [VP] * 4) and spellings["lws_handles"][1] == ["lws_handle", "lws_pool_handle", "lws_handle *", "lws_pool_handle *"]
    assert protos["lws_pointers"] == (I, [VP] * 7)
    assert spellings["lws_pointers"][1] == ["const float *", "float *", "const uint8_t *", "uint16_t *", "const lws_thing *", "double *", "void *"]
    assert protos["lws_arrays"] == (I, [VP * 4, VP * 3, VP * 2])
    assert spellings["lws_arrays"][1] == ["const float *const [4]", "float *const [3]", "uint8_t * [2]"]
    assert protos["lws_three_lines"] == (I, [VP, I, I, I, VP])


@pytest.mark.parametrize("decl,words", [
    ("int lws_f(int B, unsigned n);", ("lws_f", "`n`", "unknown type name `unsigned`")),        # nothing defaults to int
    ("int lws_f(const float *disp, size_t n, void *stream);", ("lws_f", "`n`", "unknown type name `size_t`")),
    ("int lws_f(float *out, int dims[3]);", ("lws_f", "`dims`", "array of non-pointers")),
    # a pointer to a pointer is refused, not mapped: the handle out-parameters are `lws_handle *`, one star
    ("int lws_f(lws_handle h, float **out);", ("lws_f", "`out`", "pointer to a pointer")),
    ("int lws_f(lws_handle **out);", ("lws_f", "`out`", "pointer to a pointer")),
    ("void lws_f(int B);", ("lws_f", "return type", "unknown type name `void`")),
    ("int lws_f(int);", ("lws_f", "cannot read `int`")),
    ("typedef enum { LWS_A, LWS_B } lws_e;", ("enum entry `LWS_A`",)),
    ("static const int lws_table[3];", ("cannot read `static const int lws_table[3]` as a function declaration",)),
])
def test_reader_refuses_what_it_cannot_map(decl, words):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(decl, "small.h")
    assert str(e.value).startswith("small.h: ")
    for w in words:
        assert w in str(e.value), str(e.value)


def test_import_without_the_header_names_the_missing_path(tmp_path):
    """_lib.py in a tree without include/lwsnet_hip.h: importing it raises and names the path; no empty table is left behind."""
    (tmp_path / "pkg").mkdir()
    shutil.copy(_lib.__file__, tmp_path / "pkg" / "_lib.py")
    spec = importlib.util.spec_from_file_location("lib_without_header", tmp_path / "pkg" / "_lib.py")
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "include" / "lwsnet_hip.h"))):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "lwsnet_hip.h"))


def test_call_names_the_function_once(hip_lib):
    """_lib.call: the status is checked under the name it was called by; _lib.nbytes: a negative size is a status."""
    rc, h = _create(hip_lib)
    assert rc == 0
    _lib.call("lws_set_option", h, b"fork2_after", 2)
    v = ctypes.c_int(0)
    _lib.call("lws_get_option", h, b"fork2_after", ctypes.byref(v))
    assert v.value == 2
    with pytest.raises(ValueError, match="unknown option"):
        _lib.call("lws_set_option", h, b"bogus", 1)
    with pytest.raises(RuntimeError, match=r"^lws_finalize: .* \(status -3\)$"):
        _lib.call("lws_finalize", h)
    with pytest.raises(AttributeError):
        _lib.call("lws_no_such_function", h)
    _lib.call("lws_destroy", h)
    assert _lib.nbytes("lws_surface_mesh_workspace", 1, 1) == 512
    with pytest.raises(ValueError, match="surface_mesh_workspace: bad shape B=0 H=368"):
        _lib.nbytes("lws_surface_mesh_workspace", 0, 368)


def test_library_exports_every_symbol(hip_lib):
    for name in _declared():
        assert hasattr(hip_lib, name), name
    assert hip_lib.lws_abi_version() == 8


def _create(lib, **kw):
    a = default_args(**kw)
    cfg = _lib.LwsConfig((ctypes.c_int32 * 3)(*a.maxdisplist), a.layers_3d, a.channels_3d,
                         (ctypes.c_int32 * 3)(*a.growth_rate), 0, a.interp_align_mode)
    h = ctypes.c_void_p()
    rc = lib.lws_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


def test_create_rejects_unsupported_config(hip_lib):
    rc, _ = _create(hip_lib, channels_3d=5)
    assert rc == _lib.LWS_ERR_INVALID
    with pytest.raises(ValueError, match="not supported"):
        _lib.check(rc)
    rc, _ = _create(hip_lib, maxdisplist=(100, 5, 5))
    assert rc == _lib.LWS_ERR_INVALID
    rc, _ = _create(hip_lib, interp_align_mode=2)          # lws_config.interp_align_mode (ABI v8): 0 or 1
    assert rc == _lib.LWS_ERR_INVALID and b"interp_align_mode" in hip_lib.lws_last_error()
    rc, h = _create(hip_lib, interp_align_mode=1)
    assert rc == 0
    hip_lib.lws_destroy(h)


def test_set_tensor_validates_keys_and_shapes(hip_lib):
    rc, h = _create(hip_lib)
    assert rc == 0
    sd = make_state_dict(7)
    k = "volume_postprocess.0.1.2.weight"
    v = sd[k]
    shp = (ctypes.c_int64 * v.ndim)(*v.shape)
    assert hip_lib.lws_set_tensor(h, k.encode(), v.ctypes.data_as(_lib.c_float_p), shp, v.ndim) == 0
    assert hip_lib.lws_set_tensor(h, b"no.such.key", v.ctypes.data_as(_lib.c_float_p), shp, v.ndim) == _lib.LWS_ERR_INVALID
    assert b"unexpected key" in hip_lib.lws_last_error()
    bad = (ctypes.c_int64 * 2)(3, 3)
    assert hip_lib.lws_set_tensor(h, k.encode(), v.ctypes.data_as(_lib.c_float_p), bad, 2) == _lib.LWS_ERR_INVALID
    assert b"shape mismatch" in hip_lib.lws_last_error()
    # finalize without the full state dict is a state error, not a crash
    assert hip_lib.lws_finalize(h) == _lib.LWS_ERR_STATE
    with pytest.raises(RuntimeError):
        _lib.check(_lib.LWS_ERR_STATE, "lws_finalize")
    assert hip_lib.lws_destroy(h) == 0


@pytest.mark.parametrize("kw", [{}, dict(maxdisplist=(8, 1, 1), layers_3d=1, channels_3d=16, growth_rate=(1, 1, 1)),
                                dict(maxdisplist=(30, 5, 5), layers_3d=4, channels_3d=8, growth_rate=(4, 4, 4))],
                         ids=["default", "c3=16,layers=1", "c3=32x3,layers=4"])
def test_set_tensor_accepts_the_python_spec(hip_lib, kw):
    """The library's key table against lwsnet_amd/weights.py:state_dict_spec, the independent statement of the contract:
    every (key, shape) of the spec is accepted, the same key with its last dimension + 1 is refused."""
    from lwsnet_amd.weights import state_dict_spec
    rc, h = _create(hip_lib, **kw)
    assert rc == 0
    for key, shape, _ in state_dict_spec(default_args(**kw)):
        v = np.zeros(shape[:-1] + (shape[-1] + 1,), np.float32)
        shp = (ctypes.c_int64 * len(shape))(*shape)
        assert hip_lib.lws_set_tensor(h, key.encode(), v.ctypes.data_as(_lib.c_float_p), shp, len(shape)) == 0, key
        bad = (ctypes.c_int64 * len(shape))(*v.shape)
        assert hip_lib.lws_set_tensor(h, key.encode(), v.ctypes.data_as(_lib.c_float_p), bad, len(shape)) == _lib.LWS_ERR_INVALID, key
        assert b"shape mismatch" in hip_lib.lws_last_error(), key
    assert hip_lib.lws_destroy(h) == 0


def test_model_shim_validates_on_host(hip_lib):
    from lwsnet_amd.models import LWSNet
    m = LWSNet(default_args(), device=None) if False else None   # constructed below without a device
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-only behaviour")
    m = LWSNet(default_args())
    assert m.eval() is m
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(KeyError):
        m.set_state_dict({"feature_extraction.dres0.0.0.weight": np.zeros((4, 3, 3, 3), np.float32)})
    sd = make_state_dict(7)
    sd["StructuredToParameterName@@"] = {}
    m.set_state_dict(sd)                      # host-side ingest works without a GPU
    assert len(m.state_dict()) == 226
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(np.zeros((1, 3, 64, 256), np.float32), np.zeros((1, 3, 64, 256), np.float32))


def test_check_size_matches_reference_constraints():
    from lwsnet_amd.synth import check_size
    check_size(256, 512)
    check_size(368, 1232)
    check_size(544, 960, 32)
    for H, W in ((375, 1242), (540, 960), (256, 128)):
        with pytest.raises(ValueError):
            check_size(H, W)


def test_options_validate_names_and_ranges(hip_lib):
    """lws_set_option / lws_get_option are host-side: they work without a GPU."""
    rc, h = _create(hip_lib)
    assert rc == 0
    v = ctypes.c_int(123)
    for name, default in [(b"fuse_first", 3), (b"defer_upsample", 1), (b"side_streams", 1), (b"split_bf16", 0), (b"ref_chunk_mb", 72),
                          (b"ref_pipe", -1), (b"warp_form", 1), (b"fuse_last1", 1), (b"fork2_after", -1), (b"fuse_ref_last", -1)]:
        assert hip_lib.lws_get_option(h, name, ctypes.byref(v)) == 0 and v.value == default
    assert hip_lib.lws_set_option(h, b"fork2_after", 2) == 0
    assert hip_lib.lws_get_option(h, b"fork2_after", ctypes.byref(v)) == 0 and v.value == 2
    assert hip_lib.lws_set_option(h, b"fork2_after", 17) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_set_option(h, b"fuse_first", 4) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_set_option(h, b"warp_form", 2) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_set_option(h, b"bogus", 1) == _lib.LWS_ERR_INVALID
    assert b"unknown option" in hip_lib.lws_last_error()
    # ABI v8 retired the options two rounds of sweeps had shown to tie or lose, and the per-kernel forms of the numerics mode
    for name in (b"left_at", b"split_heads", b"fuse_shift", b"conv3d_order", b"mid8_tile", b"mid8_balance", b"fork_ext", b"tail_at",
                 b"mid8_form", b"mid16_form", b"conv64_form"):
        assert hip_lib.lws_set_option(h, name, 0) == _lib.LWS_ERR_INVALID and hip_lib.lws_get_option(h, name, ctypes.byref(v)) == _lib.LWS_ERR_INVALID
    # the opt-in numerics mode: a bit per MFMA convolution that has a split-bf16 form
    for mask in (1, 2, 4, 7, 0):
        assert hip_lib.lws_set_option(h, b"split_bf16", mask) == 0
        assert hip_lib.lws_get_option(h, b"split_bf16", ctypes.byref(v)) == 0 and v.value == mask
    assert hip_lib.lws_set_option(h, b"split_bf16", 8) == _lib.LWS_ERR_INVALID
    hip_lib.lws_destroy(h)


def test_handle_refuses_a_foreign_current_device(hip_lib):
    """include/lwsnet_hip.h: a handle belongs to one HIP device and every GPU-touching call checks that it is the calling
    thread's current device (a launch from another device would run on foreign pointers).  Host-side check: it fires
    before any HIP work, so it is testable without a GPU -- rebind the handle to device 5 (legal before anything is
    allocated) and call in from whatever device is current here (-1 on a CPU box, 0 on the one-GPU box)."""
    rc, h = _create(hip_lib)
    assert rc == 0
    v = ctypes.c_int(99)
    assert hip_lib.lws_get_option(h, b"device", ctypes.byref(v)) == 0 and v.value in (-1, 0)
    assert hip_lib.lws_set_option(h, b"device", -3) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_set_option(h, b"device", 5) == 0
    assert hip_lib.lws_reserve(h, 1, 64, 256) == _lib.LWS_ERR_INVALID
    msg = hip_lib.lws_last_error()
    assert b"belongs to HIP device 5" in msg and b"current device" in msg
    with pytest.raises(ValueError, match="belongs to HIP device 5"):
        _lib.check(_lib.LWS_ERR_INVALID)
    z = np.zeros((1, 3, 64, 256), np.float32)
    outs = (ctypes.c_void_p * 4)(*[z.ctypes.data] * 4)
    assert hip_lib.lws_forward(h, z.ctypes.data, z.ctypes.data, 1, 64, 256, outs, None) == _lib.LWS_ERR_INVALID
    assert b"lws_forward: the handle belongs to HIP device 5" in hip_lib.lws_last_error()
    assert hip_lib.lws_finalize(h) == _lib.LWS_ERR_INVALID          # device check comes before the state check
    # size errors still win over the device error (pure argument validation comes first)
    assert hip_lib.lws_reserve(h, 1, 375, 1242) == _lib.LWS_ERR_INVALID
    assert b"unsupported input size" in hip_lib.lws_last_error()
    assert hip_lib.lws_destroy(h) == 0


def test_clone_and_pool_validate_on_host(hip_lib):
    """lws_clone / lws_pool_* argument and state errors need no GPU."""
    rc, h = _create(hip_lib)
    assert rc == 0
    c = ctypes.c_void_p()
    assert hip_lib.lws_clone(h, ctypes.byref(c)) == _lib.LWS_ERR_STATE         # not finalized
    assert b"not been finalized" in hip_lib.lws_last_error()
    p = ctypes.c_void_p()
    assert hip_lib.lws_pool_create(h, 0, 0, ctypes.byref(p)) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_pool_create(h, 3, 8, ctypes.byref(p)) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_pool_create(h, 3, 0, ctypes.byref(p)) == _lib.LWS_ERR_STATE
    assert hip_lib.lws_pool_workers(None) == 0 and hip_lib.lws_pool_destroy(None) == 0
    assert hip_lib.lws_pool_wait_all(None) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_pool_clear_error(None) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_destroy(h) == 0

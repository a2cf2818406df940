"""The C ABI is written once, in include/gsraster.h: gscream_amd/_abi.py reads it, _native.py derives the binding from that reading.
Here: the reader on header text written in the test; every function of the real header against the built library and the binding;
every struct of the header against the hand-written ctypes classes and numpy dtypes; the constants the wrappers use.  CPU only."""
import ctypes

import numpy as np
import pytest

from gscream_amd import _abi, _native, png_decode

ABI = _abi.header()

SAMPLE = """
/* a header in the style of gsraster.h */
#ifndef SAMPLE_H
#define SAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef enum gsr_status { GSR_OK = 0, GSR_ERR_HIP = -2, /* int gsr_not_a_function(int x); */ GSR_NEED_CAPACITY = 1 } gsr_status;
enum { GSR_STAGE_A = 0, GSR_STAGE_B, GSR_STAGE_C = 5, GSR_STAGE_D, GSR_NUM_STAGES };
#define GSR_ABI_VERSION 8
#define GSR_PIECE_START 2u
#define GSR_MASK 0x10
#define GSR_NOT_A_NUMBER (1 << 3)
typedef struct gsr_profile {
    double total_ms[GSR_NUM_STAGES];   /* per stage */
    int64_t launches[3];
} gsr_profile;
typedef struct {
    const float* src;  // device
    long long stride_b, stride_c;
    int32_t x0, width;
} gsr_panel;
const char* gsr_version(void);
void gsr_reset(void);
size_t gsr_bytes(unsigned mask, long long stride, uint64_t seed);
int gsr_decode(int N, const float* const* weights /* host array */,
               float* const* grads16,   // host array
               const gsr_panel* panels /* host */, gsr_profile* out_host,
               const void* geom, double eps,
               void* stream /* hipStream_t */);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_functions():
    f = _abi.parse(SAMPLE).functions
    assert list(f) == ["gsr_version", "gsr_reset", "gsr_bytes", "gsr_decode"], "a prototype inside a comment is no declaration"
    assert f["gsr_version"] == ("const char*", []) and f["gsr_reset"] == ("void", [])
    assert f["gsr_bytes"] == ("size_t", [("unsigned", "mask", False, False), ("long long", "stride", False, False),
                                         ("uint64_t", "seed", False, False)])
    assert f["gsr_decode"] == ("int", [("int", "N", False, False), ("const float* const*", "weights", True, True),
                                       ("float* const*", "grads16", True, False), ("const gsr_panel*", "panels", True, True),
                                       ("gsr_profile*", "out_host", True, False), ("const void*", "geom", True, True),
                                       ("double", "eps", False, False), ("void*", "stream", True, False)])


def test_reader_constants_and_structs():
    abi = _abi.parse(SAMPLE)
    assert abi.constants == {"GSR_OK": 0, "GSR_ERR_HIP": -2, "GSR_NEED_CAPACITY": 1, "GSR_STAGE_A": 0, "GSR_STAGE_B": 1, "GSR_STAGE_C": 5,
                             "GSR_STAGE_D": 6, "GSR_NUM_STAGES": 7, "GSR_ABI_VERSION": 8, "GSR_PIECE_START": 2, "GSR_MASK": 16}
    assert abi.structs == {"gsr_profile": [("double", "total_ms", 7), ("int64_t", "launches", 3)],
                           "gsr_panel": [("const float*", "src", None), ("long long", "stride_b", None), ("long long", "stride_c", None),
                                         ("int32_t", "x0", None), ("int32_t", "width", None)]}


def test_type_map_and_the_types_it_refuses():
    class Panel(ctypes.Structure):
        _fields_ = [("src", ctypes.c_void_p)]
    structs = {"gsr_panel": Panel}
    want = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint64_t": ctypes.c_uint64,
            "int64_t": ctypes.c_int64, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const float* const*": ctypes.c_void_p,
            "float* const*": ctypes.c_void_p, "const gsr_panel*": ctypes.POINTER(Panel), "gsr_panel*": ctypes.POINTER(Panel),
            "gsr_panel* const*": ctypes.c_void_p, "const gsr_other*": ctypes.c_void_p}
    for decl, t in want.items():
        assert _abi.ctype(decl, structs) is t, decl
    assert _abi.ctype("void", returns=True) is None and _abi.ctype("const char*", returns=True) is ctypes.c_char_p
    assert _abi.ctype("size_t", returns=True) is ctypes.c_size_t
    for decl, returns in (("short", False), ("long", False), ("gsr_status", False), ("bool", True), ("void", False), ("float*", True)):
        with pytest.raises(TypeError, match="no ctypes type"):  # never a quiet int
            _abi.ctype(decl, structs, returns=returns)
    with pytest.raises(KeyError):
        _abi.parse("typedef struct gsr_s { int v[GSR_UNDECLARED]; } gsr_s;")


def test_header_is_read_once_and_a_missing_one_is_fatal(monkeypatch, tmp_path):
    assert _abi.header() is ABI is _native._ABI
    monkeypatch.setattr(_abi, "_header", None)
    monkeypatch.setattr(_abi, "HEADER_PATH", str(tmp_path / "gsraster.h"))
    with pytest.raises(RuntimeError, match=r"gsraster\.h cannot be read"):
        _abi.header()


def test_the_real_header_as_a_whole(native_lib):
    assert len(ABI.functions) == 86 and _native.EXPORTED_SYMBOLS == tuple(ABI.functions)
    assert ABI.constants["GSR_ABI_VERSION"] == _native.ABI_VERSION == native_lib.gsr_abi_version() == 9
    assert native_lib.gsr_version().startswith(b"gsraster")
    assert sorted(ABI.structs) == sorted(list(_native.STRUCTS) + ["gsr_png_piece", "gsr_png_file"])
    assert {k: v for k, v in ABI.constants.items() if k.startswith("GSR_ERR") or k in ("GSR_OK", "GSR_NEED_CAPACITY")} == {
        "GSR_OK": 0, "GSR_ERR_INVALID_ARGUMENT": -1, "GSR_ERR_HIP": -2, "GSR_ERR_UNSUPPORTED": -3, "GSR_ERR_NO_DEVICE": -4, "GSR_NEED_CAPACITY": 1}
    assert [ABI.constants["GSR_STAGE_" + n] for n in ("PREPROCESS", "COUNT_SCAN", "SCATTER", "TILE_SORT", "BLEND_FWD", "BLEND_BWD", "GAUSS_BWD")] \
        == list(range(7)) and ABI.constants["GSR_NUM_STAGES"] == _native.NUM_STAGES == len(_native.STAGE_NAMES) == 7
    assert [ABI.constants["GSR_PNG_" + n] for n in ("OK", "TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "BAD_CODE", "BAD_SYMBOL", "DISTANCE", "TOO_LONG",
                                                    "TOO_SHORT", "FILTER", "ADLER", "CRC", "TABLE")] == list(range(13)) and len(_native.PNG_STATUS) == 13
    for name in _native._CONSTANTS:
        assert getattr(_native, name) == ABI.constants["GSR_" + name], name


@pytest.mark.parametrize("name", list(ABI.functions))
def test_header_binding_and_library_agree(native_lib, name):
    """Every function the header declares: the library exports it, and the binding types it as declared -- as many argtypes as
    parameters, each the map's type for the declared one (a typed pointer exactly where the struct has a class), and the restype."""
    returns, params = ABI.functions[name]
    assert hasattr(native_lib, name), "the library does not export it"
    fn = getattr(native_lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params)
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
               "long long": ctypes.c_longlong, "uint64_t": ctypes.c_uint64}  # written again here: what the 86 declarations use
    typed = {"gsr_stage1_result*": _native.Stage1Result, "const gsr_tuning*": _native.Tuning, "const gsr_adjust_copy*": _native.AdjustCopy,
             "const gsr_adam_tensor*": _native.AdamTensor, "const gsr_frame_panel*": _native.FramePanel, "gsr_profile*": _native.Profile,
             "gsr_layout_piece*": _native.LayoutPiece}
    for got, (decl, pname, is_pointer, _) in zip(fn.argtypes, params):
        want = ctypes.POINTER(typed[decl]) if decl in typed else ctypes.c_void_p if is_pointer else scalars[decl]
        assert got is want, (pname, decl, got)
    assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void": None}[returns]


_NUMPY = {"int32_t": "<i4", "uint32_t": "<u4", "uint64_t": "<u8"}
_DTYPES = {"gsr_png_piece": png_decode._PIECE, "gsr_png_file": png_decode._FILE}


@pytest.mark.parametrize("name", list(ABI.structs))
def test_struct_mirrors_follow_the_header(name):
    """Field names, order, C types and array lengths of every hand-written mirror -- the seven ctypes classes, the two numpy dtypes --
    equal the header's struct; with the natural alignment both sides use, the offsets follow."""
    fields = ABI.structs[name]
    if name in _DTYPES:
        dt = _DTYPES[name]
        assert [(n, dt.fields[n][0].str) for n in dt.names] == [(f, _NUMPY[c]) for c, f, length in fields if length is None]
        assert len(dt.names) == len(fields) and dt.itemsize == sum(np.dtype(_NUMPY[c]).itemsize for c, _, _ in fields)  # no padding
        return
    cls = _native.STRUCTS[name]
    want = [(f, _abi.ctype(c) if length is None else _abi.ctype(c) * length) for c, f, length in fields]
    assert len(cls._fields_) == len(want)
    for (got_name, got_type), (want_name, want_type) in zip(cls._fields_, want):
        assert got_name == want_name and got_type is want_type, (got_name, got_type, want_name, want_type)

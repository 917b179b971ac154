"""An independent reading of include/vaw_hip.h for the tests of the C ABI binding: regular expressions of its own over the header
text, never vaw_amd._abi (the product's parser) and never a table of the package.  What the binding must look like is spelled here
from each prototype, per parameter; the tests compare the live binding (vaw_amd.lib().<name>.restype / .argtypes) with it."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "vaw_hip.h")).read(), flags=re.S)          # comments removed

# header struct -> the name of its Structure class in vaw_amd._lib
STRUCT_CLASSES = {"vaw_epilogue": "Epilogue", "vaw_wgrad_problem": "WgradProblem", "vaw_fp8_quant_job": "Fp8QuantJob",
                  "vaw_gemm_knobs": "GemmKnobs", "vaw_gemm_launch": "GemmLaunch", "vaw_gemm_fp8_launch": "GemmFp8Launch",
                  "vaw_reduce_job": "ReduceJob", "vaw_row_launch": "RowLaunch", "vaw_attn_desc": "AttnDesc", "vaw_attn_launch": "AttnLaunch",
                  "vaw_gn_launch": "GnLaunch", "vaw_conv3x3_launch": "Conv3x3Launch", "vaw_cast_colsum_launch": "CastColsumLaunch",
                  "vaw_dit_ws_plan_t": "DitWsPlan"}
ENUMS = set(re.findall(r"typedef enum \{[^}]*\} (\w+);", CODE))
STRUCTS = dict((n, body) for body, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", CODE))          # name -> field text
PROTOS = re.findall(r"\b(int|int64_t|void|const char\*)\s+(vaw_\w+)\s*\(([^)]*)\)\s*;", CODE)          # (return, name, parameter text)
KINDS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double,
         **{e: C.c_int for e in ENUMS}}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char*": C.c_char_p}


def kind(ctype, name, host=False):
    """the ctypes form of a parameter or field declared `ctype name`: scalars and enums by value, vaw_stream and device pointers
    c_void_p, a pointer to a header struct POINTER(its class), a host array (name ends in _host, or `host`) POINTER(scalar)"""
    from vaw_amd import _lib
    base = ctype.replace("const ", "").replace("*", "").strip()
    if "*" not in ctype:
        return C.c_void_p if ctype == "vaw_stream" else KINDS[ctype]
    if base in STRUCTS:
        return C.POINTER(getattr(_lib, STRUCT_CLASSES[base]))
    assert base in KINDS or base in ("void", "char"), (ctype, name)
    return C.POINTER(KINDS[base]) if (host or name.endswith("_host")) and base in KINDS else C.c_void_p


def signatures():
    """name -> (restype, [argtypes]) as the header's prototypes spell them"""
    return {name: (RETURNS[ret], [] if params.strip() == "void" else [kind(*" ".join(p.split()).rsplit(" ", 1)) for p in params.split(",")])
            for ret, name, params in PROTOS}


def assert_bound_as_declared(lib, name):
    """lib.<name> carries the restype and the argtypes of its prototype in the header, parameter by parameter"""
    want = signatures()[name]
    fn = getattr(lib, name)
    assert fn.restype is want[0] and fn.argtypes is not None and list(fn.argtypes) == want[1], (name, fn.restype, fn.argtypes, want)
    return want[1]

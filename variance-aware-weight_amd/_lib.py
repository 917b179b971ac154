"""ctypes binding of libvaw_hip.so (include/vaw_hip.h).  No fallback: if the library is missing,
or a call is made without a GPU tensor, this raises."""
import ctypes as C
import os

import torch

from ._abi import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAW_HIP_LIB") or os.path.join(_HERE, "libvaw_hip.so")   # (override: measurement builds only)


class VawError(RuntimeError):
    pass


# ---- constants: every enumerator and integer #define of the header under its C name less the VAW_ prefix ----------------------
# F32 BF16 FP8 BF8 F64 (vaw_dtype), GV_* GR_* GS_* GC_* (vaw_gemm_variant / _reduce / _rowsum_mode / _colsum_mode), CVR_* CVB_*
# (vaw_conv_reduce / _bias_grad), ROW_* RV_* (vaw_row_kind / _variant), AV_* (vaw_attn_variant), GN_* GNV_* (vaw_gn_pass / _variant),
# RESAMPLER_MAX_T, EDM_COLS, FLOW_COLS, DPM_COLS, NOISE_*, RK_STAGES, FLOW_LOGP_COLS, ...
CONSTANTS = {}
for _values in (*HEADER.enums.values(), HEADER.defines):
    for _name, _value in _values.items():
        if not _name.startswith("VAW_") or _name[4:] in CONSTANTS:
            raise VawError(f"include/vaw_hip.h: {_name} lacks the VAW_ prefix or is defined twice")
        CONSTANTS[_name[4:]] = _value
globals().update(CONSTANTS)
# the names that are not the C name less VAW_
ATTN_FWD, ATTN_BWD, ATTN_BWD_COLSUM = (CONSTANTS[n] for n in ("ATTN_DIR_FWD", "ATTN_DIR_BWD", "ATTN_DIR_BWD_COLSUM"))
TORCH_DTYPE = {CONSTANTS["F32"]: torch.float32, CONSTANTS["BF16"]: torch.bfloat16}


def _enum_names(enum, strip):
    """the enumerators of `enum` less their prefix, indexed by value"""
    return tuple(n[len(strip):] for n, _ in sorted(HEADER.enums[enum].items(), key=lambda nv: nv[1]))


AV_NAMES = tuple(n.lower() for n in _enum_names("vaw_attn_variant", "VAW_AV_"))
GV_NAMES = tuple(n.lower() for n in _enum_names("vaw_gemm_variant", "VAW_GV_"))
CVR_NAMES = _enum_names("vaw_conv_reduce", "VAW_")
CVB_NAMES = _enum_names("vaw_conv_bias_grad", "VAW_")
# the epilogue kinds of csrc/gemm_epi.h (not part of the public header)
P8_STORE, P8_GELU, P8_DGELU, P8_GATE, P8_SLAB, P8_ANY, P8_WGRAD, P8_RESID, P8_GELU_Q, P8_DGELU_Q = range(10)
P8_NAMES = ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE", "P8_SLAB", "P8_ANY", "P8_WGRAD", "P8_RESID", "P8_GELU_Q", "P8_DGELU_Q")

# ---- types: int and enums -> c_int; vaw_stream and pointers to scalars or void -> c_void_p (device addresses travel as integers),
# unless the name ends in _host, the header's mark of a host array -> POINTER(scalar); pointers to a header struct -> POINTER(it)
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double,
            **{e: C.c_int for e in HEADER.enums}}
_RETURNS = {("int", False): C.c_int, ("int64_t", False): C.c_int64, ("void", False): None, ("char", True): C.c_char_p}
# the one host pointer of a struct: in / out row count of colsum_partial_out (read and written by the host side of vaw_gemm)
_HOST_FIELDS = {("vaw_epilogue", "colsum_rows_out")}
STRUCTS = {}          # C name -> Structure class


def _ctype(t, name, owner):
    if not t.pointer:
        if t.base == "vaw_stream":
            return C.c_void_p
        if t.base in _SCALARS:
            return _SCALARS[t.base]
    elif t.base in STRUCTS:
        return C.POINTER(STRUCTS[t.base])
    elif t.base in ("void", "char") or t.base in _SCALARS:
        host = name.endswith("_host") or (owner, name) in _HOST_FIELDS
        return C.POINTER(_SCALARS[t.base]) if host and t.base in _SCALARS else C.c_void_p
    raise VawError(f"include/vaw_hip.h: no ctypes form for {t.base}{'*' if t.pointer else ''} {name} of {owner}")


# Structure classes, one per header struct, named in CamelCase less vaw_ and _t: Epilogue, AttnDesc, RowLaunch, AttnLaunch, GnLaunch,
# GemmKnobs, GemmLaunch, Conv3x3Launch, GemmFp8Launch, DitWsPlan, CastColsumLaunch, Fp8QuantJob, WgradProblem, ReduceJob
for _cname, _fields in HEADER.structs.items():
    _pyname = "".join(w.capitalize() for w in _cname[len("vaw_"):].removesuffix("_t").split("_"))
    STRUCTS[_cname] = type(_pyname, (C.Structure,), {"__doc__": f"{_cname} of include/vaw_hip.h",
                                                     "_fields_": [(f, _ctype(t, f, _cname)) for f, t in _fields]})
    globals()[_pyname] = STRUCTS[_cname]

# name -> (restype, argtypes) of every function the header declares
SIGNATURES = {}
for _name, _fn in HEADER.functions.items():
    if tuple(_fn.ret) not in _RETURNS:
        raise VawError(f"include/vaw_hip.h: no ctypes form for the return type of {_name}")
    SIGNATURES[_name] = (_RETURNS[tuple(_fn.ret)], [_ctype(t, p, _name) for t, p in _fn.params])

_lib = None


def lib():
    """Load (once) and return the CDLL with every declared function bound.  Raises if the HIP library was not built or lacks one;
    behind VAW_HIP_LIB (an older measurement build, A/B runs) the entry points added since are simply left unbound."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VawError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("VAW_HIP_LIB"):
                    continue
                raise VawError(f"{LIB_PATH} does not export {name}, which include/vaw_hip.h declares") from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def exported_symbols():
    """every function include/vaw_hip.h declares"""
    return sorted(SIGNATURES)


# VAW_STEP_FUSED (read once): 0 restores the step's unfused sequence of launches everywhere -- separate cast / column-sum
# passes in the DiT backward, tensor operations for the latent sample, the coefficient gathers and the batch means of the loss
STEP_FUSED = os.environ.get("VAW_STEP_FUSED", "1") != "0"
# VAW_ROWS_FWD_FUSED (read once): 0 restores the gated-residual epilogue of proj / fc2 followed by a LayerNorm launch of
# its own in the bf16 DiT block forward, in place of the plain store and vaw_gate_resid_ln_modulate_fwd
ROWS_FWD_FUSED = os.environ.get("VAW_ROWS_FWD_FUSED", "1") != "0"


def check(rc, what):
    if rc != 0:
        raise VawError(f"{what} failed ({rc}): {lib().vaw_last_error_string().decode()}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise VawError("vaw_amd runs on the GPU only: got a CPU tensor (no CPU fallback exists by design)")

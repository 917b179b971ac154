"""Float64 reference, per-element error bound and case table for vaw_gemm (imported by test_gemm_parity_cpu.py and
test_gpu_gemm.py; no GPU needed, tensors live wherever the caller puts them).

Reference.  Every output in float64 from the exact stored inputs (bf16 or f32 values), in the header's order
    acc*alpha + bias -> [aux_out] -> act -> *gate -> +resid -> +rowadd -> beta*C_old +
C, aux_out, colsum_out (colsum_beta * old + column sums of C AS STORED, also for the folded rows of a colsum_partial) and
rowsum_a_out (rowsum_a_beta * old + row sums of op(A)).  Where a value is saved rounded and then used -- aux_out feeds the activation
and the gate -- the reference continues from the kernel's stored aux_out (itself checked), so a rounding flip of aux_out cannot
show up as an error of C.

Bound, element by element, the same expressions in absolute values (u = 2^-24, the unit of the f32 accumulator):
    E   = K u |alpha| (|A| |B|)                      accumulation, carried through the epilogue's factors: x sup|gelu'| = 1.13 through
                                                     GELU without aux_out, x |gelu'(aux_in)|, x |gate|; 0 behind a stored aux_out
    F   = 8 u (the whole epilogue in absolute values) its f32 operations: alpha, bias, three for the activation (polynomial, exp,
                                                     reciprocal), gate, residual / row add, beta -- each rounds once at most at
                                                     the magnitude of the absolute-value expression
    R   = 2^-8 |acc| |gelu'| |gate|                  parked-drain / warp-specialised GELU': the input gradient is rounded to bf16
                                                     before the multiply (csrc/gemm_pd_kernel.h)
    C:        c (E + F) + R + s |C|                  s = 2^-8 for a bf16 C, 2^-24 for an f32 C
    aux_out:  c (E + F) + s_act |aux|
    colsum:   c (M + 2) u (|colsum_beta old| + sum_m |C stored|)
    rowsum:   c (K + 2) u (|rowsum_a_beta old| + sum_k |A|)
One constant c per dtype, C_BOUND, the same for every variant and case: 1 for both.  Worst err / bound per variant on the MI355X
(pytest -m gpu tests/test_gpu_gemm.py --junitxml): see MEASURED below and DESIGN.md.

simulate() is the comparator's own test object: the reference rounded at the stated points ("kernel output" made on the CPU), with
one injected fault at a time (FAULTS)."""
import zlib

import torch

U32 = 2.0 ** -24
UNIT = {"bf16": 2.0 ** -8, "f32": U32}
C_BOUND = {"bf16": 1.0, "f32": 1.0}
EPI_F32_OPS = 8
GELU_GRAD_SUP = 1.13              # sup |d/dx gelu_tanh(x)| = 1.1289 (x = 1.47)
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
WS_FLOATS = 1 << 26               # the grow-only scratch ops.gemm hands to vaw_gemm when the call may need one

# worst err / bound per variant on the MI355X, default process knobs, c = 1: (outputs stored as bf16, outputs stored as f32).  The
# bf16 figures sit just below 1 on every variant: the storage term is the exact half-ulp of bf16 rounding, and among a few thousand
# elements one always nearly attains it; the f32-stored outputs show the arithmetic's own share.
MEASURED = {"generic": (0.987, 0.686), "t128_bk32": (0.995, None), "t128_bk64": (0.988, 0.207), "ring256": (0.991, 0.209),
            "persistent": (0.991, 0.111), "small_m": (0.993, 0.212), "parked_drain": (0.986, 0.111), "warp_spec": (0.986, 0.111)}

P8 = ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE", "P8_SLAB", "P8_ANY", "P8_WGRAD", "P8_RESID")
TARGET_FIELDS = ("variant", "ntw", "sm", "epi_kind", "split", "reduce", "rowsum_mode", "colsum_mode", "xcd")


def rnd(x, dt):
    """x (float64) rounded to the storage format, back in float64"""
    return x.to(TORCH_DT[dt]).double()


def gelu(x):
    k0, k1 = 0.7978845608028654, 0.044715
    return 0.5 * x * (1.0 + torch.tanh(k0 * (x + k1 * x ** 3)))


def gelu_grad(x):
    k0, k1 = 0.7978845608028654, 0.044715
    t = torch.tanh(k0 * (x + k1 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * k0 * (1.0 + 3.0 * k1 * x * x)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _c(name, tile, layout, M, N, K, target, dt="bf16", generic=0, regime="normal", pad=(0, 0, 0), off=(), **epi):
    e = dict(bias=0, act=0, aux_out=0, gate=0, resid=None, rowadd=0, rpb=0, alpha=1.0, beta=0.0, out_f32=0, colsum=None,
             colsum_beta=0.0, rowsum=0, rowsum_beta=0.0)
    assert set(epi) <= set(e), (name, epi)
    e.update(epi)
    tgt = dict(zip(TARGET_FIELDS, target))
    return dict(name=name, tile=tile, ak=layout[0], bk=layout[1], M=M, N=N, K=K, dt=dt, generic=generic, regime=regime, pad=pad,
                off=tuple(off), target=tgt, **e)


BIAS = dict(bias=1)
GELU = dict(bias=1, act=1, aux_out=1)
DGELU = dict(act=2)
DGELU_CS = dict(act=2, colsum="out", colsum_beta=0.5)
GATE = dict(bias=1, aux_out=1, gate=1, resid="f32", out_f32=1, rpb=24)
GATE27 = dict(GATE, rpb=27)
RESID = dict(bias=1, resid="act")
ROWADD = dict(bias=1, rowadd=1, rpb=24)
AB = dict(bias=1, alpha=0.25, beta=0.5, out_f32=1)
CS_PART = dict(colsum="partial")
CS_OUT = dict(bias=1, colsum="out", colsum_beta=0.5)
PAD = (8, 16, 8)

# target = (variant, ntw, (mb, nb, stages), epi_kind, split > 1, reduce, rowsum_mode, colsum_mode, XCD-mapped split)
_SPECS = [
    # ---- 128 x 128 (tile 0; by shape for the 32-deep stage) ----
    ("t128_alpha_beta", 0, (1, 1), 200, 72, 64, AB, {}),
    ("t128_bk32_by_shape", -1, (1, 0), 12296, 1032, 64, BIAS, {}),
    ("t128_split16_f32_beta", 0, (0, 0), 256, 256, 4096, dict(out_f32=1, beta=1.0), {}),
    ("t128_split_bf16_xcd", 0, (1, 1), 136, 72, 2048, {}, {}),
    ("t128_split_alpha_beta", 0, (0, 0), 264, 200, 2048, dict(out_f32=1, alpha=0.25, beta=0.5), {}),
    ("t128_rowsum_split8", 0, (0, 0), 264, 200, 2048, dict(out_f32=1, rowsum=1, rowsum_beta=2.0), {}),
    ("t128_rowsum_nosplit", 0, (0, 0), 264, 200, 64, dict(out_f32=1, beta=1.0, rowsum=1), {}),
    ("t128_rowsum_colsum", 0, (0, 0), 264, 200, 128, dict(out_f32=1, rowsum=1, colsum="out"), {}),
    ("t128_gelu_wide", 0, (1, 1), 200, 72, 128, GELU, dict(regime="wide")),
    ("t128_gelu_cancel", 0, (1, 1), 200, 72, 256, GELU, dict(regime="cancel")),
    ("t128_dgelu_colsum", 0, (1, 0), 200, 72, 128, DGELU_CS, dict(regime="wide")),
    ("t128_gate_rpb27", 0, (1, 1), 270, 200, 128, GATE27, {}),
    ("t128_gate_rpb27_under_tile10", 10, (1, 1), 270, 200, 768, GATE27, {}),
    ("t128_resid_act", 0, (1, 1), 200, 72, 128, RESID, {}),
    ("t128_rowadd", 0, (1, 1), 200, 72, 128, ROWADD, {}),
    ("t128_layout01_bias", 0, (0, 1), 200, 72, 128, BIAS, {}),
    ("t128_ld_padded", 0, (1, 1), 200, 72, 128, GELU, dict(pad=PAD)),
    ("t128_colsum_partial_edge", 0, (1, 0), 200, 72, 128, CS_PART, {}),
    ("t128_colsum_beta", 0, (1, 1), 200, 72, 128, CS_OUT, {}),
    # ---- 256 x 256 ring (tile 1) ----
    ("ring_gelu_edges", 1, (1, 1), 264, 520, 128, GELU, dict(regime="wide")),
    ("ring_split16", 1, (0, 0), 256, 256, 4096, dict(out_f32=1), {}),
    ("ring_alpha_beta", 1, (1, 1), 264, 200, 128, AB, {}),
    ("ring_dgelu_colsum", 1, (1, 0), 264, 200, 128, DGELU_CS, dict(regime="wide")),
    ("ring_gate_rpb27", 1, (1, 1), 270, 200, 128, GATE27, {}),
    ("ring_resid_act", 1, (1, 1), 264, 200, 128, RESID, {}),
    ("ring_rowadd", 1, (1, 1), 264, 200, 128, ROWADD, {}),
    ("ring_layout01_bias", 1, (0, 1), 264, 200, 128, BIAS, {}),
    ("ring_layout00_cancel", 1, (0, 0), 264, 200, 256, dict(out_f32=1), dict(regime="cancel")),
    ("ring_ld_padded", 1, (1, 1), 264, 200, 128, GELU, dict(pad=PAD)),
    ("ring_colsum_partial_edge", 1, (1, 0), 264, 200, 128, CS_PART, {}),
    # ---- persistent (tile 2: 256 columns, 3: 192, 4: by shape) ----
    ("p8_slab_f32", 2, (0, 0), 264, 200, 4096, dict(out_f32=1), {}),
    ("p8_slab_bf16_reduce", 4, (1, 0), 8192, 768, 3072, {}, {}),
    ("p8_slab_beta_ntw3", 3, (0, 0), 264, 200, 4096, dict(out_f32=1, beta=0.5, alpha=0.25), {}),
    ("p8_any_rowadd", 2, (1, 1), 264, 200, 128, ROWADD, {}),
    ("p8_any_rowadd_ntw3", 3, (1, 1), 264, 200, 128, ROWADD, {}),
    ("p8_any_alpha_beta", 2, (1, 1), 264, 200, 128, AB, {}),
    ("p8_any_gelu_f32out_ntw3", 3, (1, 1), 264, 200, 128, dict(bias=1, act=1, out_f32=1), dict(regime="wide")),
    ("p8_resid_ntw3", 3, (1, 1), 264, 200, 128, RESID, {}),
    ("p8_resid_ntw4", 2, (1, 1), 264, 200, 128, RESID, {}),
    ("p8_gate_rpb27", 2, (1, 1), 270, 200, 128, GATE27, {}),
    ("p8_gate_ntw3", 3, (1, 1), 264, 200, 128, GATE, {}),
    ("p8_store_ntw4", 2, (1, 1), 264, 200, 128, BIAS, {}),
    ("p8_store_ntw3_colsum_beta", 3, (1, 1), 264, 200, 128, CS_OUT, {}),
    ("p8_store_layout01", 2, (0, 1), 264, 200, 128, BIAS, {}),
    ("p8_store_layout00_f32", 3, (0, 0), 264, 200, 128, dict(out_f32=1, alpha=0.25), {}),
    ("p8_gelu_ntw4_wide", 2, (1, 1), 264, 200, 128, GELU, dict(regime="wide")),
    ("p8_gelu_ntw3_cancel", 3, (1, 1), 264, 200, 256, GELU, dict(regime="cancel")),
    ("p8_dgelu_ntw4_colsum", 2, (1, 0), 264, 200, 128, DGELU_CS, dict(regime="wide")),
    ("p8_dgelu_ntw3", 3, (1, 0), 264, 200, 128, DGELU, dict(regime="wide")),
    ("p8_ld_padded", 2, (1, 1), 264, 200, 128, GATE, dict(pad=PAD)),
    ("p8_colsum_partial_edge", 2, (1, 0), 264, 200, 128, CS_PART, {}),
    # ---- parked-drain (tile 10: 256 columns, 11: 192) and warp-specialised (13 / 14); K = 768 is their minimum ----
    ("pd_store_ntw4", 10, (1, 1), 264, 200, 768, BIAS, {}),
    ("pd_store_ntw3_colsum_partial", 11, (1, 0), 264, 200, 768, CS_PART, {}),
    ("pd_gelu_ntw4_wide", 10, (1, 1), 264, 200, 768, GELU, dict(regime="wide")),
    ("pd_gelu_ntw3_cancel", 11, (1, 1), 264, 200, 768, GELU, dict(regime="cancel")),
    ("pd_dgelu_ntw4_colsum", 10, (1, 0), 264, 200, 768, DGELU_CS, dict(regime="wide")),
    ("pd_dgelu_ntw3", 11, (1, 0), 264, 200, 768, DGELU, dict(regime="wide")),
    ("pd_gate_ntw4", 10, (1, 1), 264, 200, 768, GATE, {}),
    ("pd_gate_ntw3", 11, (1, 1), 264, 200, 768, GATE, {}),
    ("pd_ld_padded", 10, (1, 1), 264, 200, 768, GATE, dict(pad=PAD)),
    ("ws_store_ntw4_colsum_beta", 13, (1, 1), 264, 200, 768, CS_OUT, {}),
    ("ws_store_ntw3", 14, (1, 0), 264, 200, 768, {}, {}),
    ("ws_gelu_ntw4_cancel", 13, (1, 1), 264, 200, 768, GELU, dict(regime="cancel")),
    ("ws_gelu_ntw3_wide", 14, (1, 1), 264, 200, 768, GELU, dict(regime="wide")),
    ("ws_dgelu_ntw4", 13, (1, 0), 264, 200, 768, DGELU, dict(regime="wide")),
    ("ws_dgelu_ntw3_colsum", 14, (1, 0), 264, 200, 768, DGELU_CS, dict(regime="wide")),
    ("ws_gate_ntw4", 13, (1, 1), 264, 200, 768, GATE, {}),
    ("ws_gate_ntw3", 14, (1, 1), 264, 200, 768, GATE, {}),
    ("ws_ld_padded", 14, (1, 1), 264, 200, 768, GELU, dict(pad=PAD)),
    # ---- small-M ring (tile 5: by shape, 6: 64 x 64, 7: 64 x 128, 8: 128 x 128) ----
    ("sm64_gelu_3stages", 6, (1, 1), 1100, 1032, 128, GELU, dict(regime="wide")),
    ("sm64_bias_4stages", 6, (1, 1), 200, 72, 128, BIAS, {}),
    ("sm_by_shape_gelu", 5, (1, 1), 200, 72, 128, GELU, {}),
    ("sm64x128_gate_rpb27", 7, (1, 1), 270, 264, 128, GATE27, {}),
    ("sm64x128_dgelu_colsum", 7, (1, 0), 200, 264, 128, DGELU_CS, dict(regime="wide")),
    ("sm64x128_resid_act", 7, (1, 1), 200, 264, 128, RESID, {}),
    ("sm64x128_rowadd", 7, (1, 1), 200, 264, 128, ROWADD, {}),
    ("sm64x128_alpha_beta", 7, (1, 1), 200, 264, 128, AB, {}),
    ("sm64x128_cancel", 7, (1, 1), 200, 264, 256, GELU, dict(regime="cancel")),
    ("sm64_colsum_partial_edge", 6, (1, 0), 200, 72, 128, CS_PART, {}),
    ("sm64_ld_padded", 6, (1, 1), 200, 72, 128, GELU, dict(pad=PAD)),
    ("sm128_dgelu", 8, (1, 0), 200, 264, 192, DGELU, dict(regime="wide")),
    ("sm128_gelu", 8, (1, 1), 200, 264, 192, GELU, {}),
    ("sm128_gate", 8, (1, 1), 200, 264, 192, GATE, {}),
    # ---- generic kernel, bf16: odd sizes, forced, misaligned operands ----
    ("gen16_gelu", -1, (1, 1), 70, 44, 24, GELU, dict(regime="wide")),
    ("gen16_gate_rpb10", -1, (1, 1), 70, 44, 24, dict(GATE, rpb=10), {}),
    ("gen16_resid_act", -1, (1, 0), 70, 45, 23, RESID, {}),
    ("gen16_rowadd", -1, (0, 1), 70, 45, 23, dict(ROWADD, rpb=10), {}),
    ("gen16_alpha_beta", -1, (0, 0), 70, 45, 23, AB, {}),
    ("gen16_dgelu_colsum", -1, (1, 0), 70, 44, 24, DGELU_CS, dict(regime="wide")),
    ("gen16_colsum_partial", -1, (1, 0), 70, 44, 24, CS_PART, {}),
    ("gen16_rowsum", -1, (0, 0), 70, 44, 24, dict(out_f32=1, rowsum=1, rowsum_beta=2.0), {}),
    ("gen16_forced_gelu", 0, (1, 1), 200, 72, 128, GELU, dict(generic=1)),
    ("gen16_forced_cancel", 0, (1, 1), 200, 72, 256, GATE, dict(generic=1, regime="cancel")),
    ("gen16_A_off2", 0, (1, 1), 200, 72, 128, GELU, dict(off=("A",))),
    ("gen16_C_off2", 0, (1, 1), 200, 72, 128, RESID, dict(off=("C",))),
    ("gen16_aux_off2", 0, (1, 1), 200, 72, 128, GATE, dict(off=("aux_out",))),
    # ---- generic kernel, f32: every epilogue, a K-split launch ----
    ("gen32_gelu", -1, (1, 1), 70, 44, 24, GELU, dict(dt="f32", regime="wide")),
    ("gen32_gate_rpb10", -1, (1, 1), 70, 44, 24, dict(GATE, rpb=10), dict(dt="f32")),
    ("gen32_resid", -1, (1, 0), 70, 45, 23, RESID, dict(dt="f32")),
    ("gen32_rowadd", -1, (0, 1), 70, 45, 23, dict(ROWADD, rpb=10), dict(dt="f32")),
    ("gen32_alpha_beta", -1, (0, 0), 70, 45, 23, AB, dict(dt="f32")),
    ("gen32_dgelu_colsum", -1, (1, 0), 70, 44, 24, DGELU_CS, dict(dt="f32", regime="wide")),
    ("gen32_rowsum", -1, (0, 0), 70, 44, 24, dict(rowsum=1, rowsum_beta=2.0), dict(dt="f32")),
    ("gen32_split_beta", -1, (0, 0), 72, 44, 4100, dict(beta=0.5, alpha=0.25), dict(dt="f32")),
    ("gen32_ld_padded_cancel", -1, (1, 1), 70, 44, 256, GATE, dict(dt="f32", pad=PAD, regime="cancel")),
]

# The launch each case must reach (default knobs, 256 CUs), written out so that a change of the plan, or of a shape, that loses
# a kernel fails test_gemm_parity_cpu.py instead of passing silently on another kernel.
_TARGETS = {
    "t128_alpha_beta": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_bk32_by_shape": ('t128_bk32', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_split16_f32_beta": ('t128_bk64', None, None, None, True, 'GR_F32', 'GS_NONE', 'GC_NONE', False),
    "t128_split_bf16_xcd": ('t128_bk64', None, None, None, True, 'GR_BF16', 'GS_NONE', 'GC_NONE', True),
    "t128_split_alpha_beta": ('t128_bk64', None, None, None, True, 'GR_F32', 'GS_NONE', 'GC_NONE', True),
    "t128_rowsum_split8": ('t128_bk64', None, None, None, True, 'GR_F32_ROWSUM', 'GS_FUSED', 'GC_NONE', True),
    "t128_rowsum_nosplit": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_FUSED', 'GC_NONE', None),
    "t128_rowsum_colsum": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_SEPARATE', 'GC_FOLD', None),
    "t128_gelu_wide": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_gelu_cancel": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_dgelu_colsum": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "t128_gate_rpb27": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_gate_rpb27_under_tile10": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_resid_act": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_rowadd": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_layout01_bias": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_ld_padded": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "t128_colsum_partial_edge": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_DEFERRED', None),
    "t128_colsum_beta": ('t128_bk64', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "ring_gelu_edges": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_split16": ('ring256', None, None, None, True, 'GR_F32', 'GS_NONE', 'GC_NONE', False),
    "ring_alpha_beta": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_dgelu_colsum": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "ring_gate_rpb27": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_resid_act": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_rowadd": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_layout01_bias": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_layout00_cancel": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_ld_padded": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ring_colsum_partial_edge": ('ring256', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_DEFERRED', None),
    "p8_slab_f32": ('persistent', 4, None, 'P8_SLAB', True, 'GR_F32', 'GS_NONE', 'GC_NONE', False),
    "p8_slab_bf16_reduce": ('persistent', 3, None, 'P8_SLAB', True, 'GR_BF16', 'GS_NONE', 'GC_NONE', False),
    "p8_slab_beta_ntw3": ('persistent', 3, None, 'P8_SLAB', True, 'GR_F32', 'GS_NONE', 'GC_NONE', False),
    "p8_any_rowadd": ('persistent', 4, None, 'P8_ANY', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_any_rowadd_ntw3": ('persistent', 3, None, 'P8_ANY', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_any_alpha_beta": ('persistent', 4, None, 'P8_ANY', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_any_gelu_f32out_ntw3": ('persistent', 3, None, 'P8_ANY', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_resid_ntw3": ('persistent', 3, None, 'P8_RESID', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_resid_ntw4": ('persistent', 4, None, 'P8_RESID', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_gate_rpb27": ('persistent', 4, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_gate_ntw3": ('persistent', 3, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_store_ntw4": ('persistent', 4, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_store_ntw3_colsum_beta": ('persistent', 3, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "p8_store_layout01": ('persistent', 4, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_store_layout00_f32": ('persistent', 3, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_gelu_ntw4_wide": ('persistent', 4, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_gelu_ntw3_cancel": ('persistent', 3, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_dgelu_ntw4_colsum": ('persistent', 4, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "p8_dgelu_ntw3": ('persistent', 3, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_ld_padded": ('persistent', 4, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "p8_colsum_partial_edge": ('persistent', 4, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_DEFERRED', None),
    "pd_store_ntw4": ('parked_drain', 4, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_store_ntw3_colsum_partial": ('parked_drain', 3, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_DEFERRED', None),
    "pd_gelu_ntw4_wide": ('parked_drain', 4, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_gelu_ntw3_cancel": ('parked_drain', 3, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_dgelu_ntw4_colsum": ('parked_drain', 4, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "pd_dgelu_ntw3": ('parked_drain', 3, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_gate_ntw4": ('parked_drain', 4, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_gate_ntw3": ('parked_drain', 3, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "pd_ld_padded": ('parked_drain', 4, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_store_ntw4_colsum_beta": ('warp_spec', 4, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "ws_store_ntw3": ('warp_spec', 3, None, 'P8_STORE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_gelu_ntw4_cancel": ('warp_spec', 4, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_gelu_ntw3_wide": ('warp_spec', 3, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_dgelu_ntw4": ('warp_spec', 4, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_dgelu_ntw3_colsum": ('warp_spec', 3, None, 'P8_DGELU', False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "ws_gate_ntw4": ('warp_spec', 4, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_gate_ntw3": ('warp_spec', 3, None, 'P8_GATE', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "ws_ld_padded": ('warp_spec', 3, None, 'P8_GELU', False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64_gelu_3stages": ('small_m', None, (1, 1, 3), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64_bias_4stages": ('small_m', None, (1, 1, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm_by_shape_gelu": ('small_m', None, (1, 1, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64x128_gate_rpb27": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64x128_dgelu_colsum": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_FOLD', None),
    "sm64x128_resid_act": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64x128_rowadd": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64x128_alpha_beta": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64x128_cancel": ('small_m', None, (1, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm64_colsum_partial_edge": ('small_m', None, (1, 1, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_DEFERRED', None),
    "sm64_ld_padded": ('small_m', None, (1, 1, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm128_dgelu": ('small_m', None, (2, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm128_gelu": ('small_m', None, (2, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "sm128_gate": ('small_m', None, (2, 2, 4), None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_gelu": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_gate_rpb10": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_resid_act": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_rowadd": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_alpha_beta": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_dgelu_colsum": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_SEPARATE', None),
    "gen16_colsum_partial": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_SEPARATE', None),
    "gen16_rowsum": ('generic', None, None, None, False, 'GR_NONE', 'GS_SEPARATE', 'GC_NONE', None),
    "gen16_forced_gelu": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_forced_cancel": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_A_off2": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_C_off2": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen16_aux_off2": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_gelu": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_gate_rpb10": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_resid": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_rowadd": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_alpha_beta": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
    "gen32_dgelu_colsum": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_SEPARATE', None),
    "gen32_rowsum": ('generic', None, None, None, False, 'GR_NONE', 'GS_SEPARATE', 'GC_NONE', None),
    "gen32_split_beta": ('generic', None, None, None, True, 'GR_F32', 'GS_NONE', 'GC_NONE', False),
    "gen32_ld_padded_cancel": ('generic', None, None, None, False, 'GR_NONE', 'GS_NONE', 'GC_NONE', None),
}


def _build_cases():
    out = {}
    for name, tile, layout, M, N, K, epi, kw in _SPECS:
        assert name not in out, name
        out[name] = _c(name, tile, layout, M, N, K, _TARGETS[name], **kw, **epi)
    return out


CASES = _build_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# geometry and inputs
# ------------------------------------------------------------------------------------------------------------------------------
def out_dt(c):
    return "f32" if (c["out_f32"] or c["dt"] == "f32") else c["dt"]


def resid_dt(c):
    return c["dt"] if c["resid"] == "act" else "f32"


def geometry(c):
    """stored shapes and leading dimensions: A [ra][ca] (lda), B [rb][cb] (ldb), C / aux / resid [M][N] (ldc), gate [samples][N] (gate_ld)"""
    M, N, K = c["M"], c["N"], c["K"]
    ra, ca = (M, K) if c["ak"] else (K, M)
    rb, cb = (N, K) if c["bk"] else (K, N)
    samples = -(-M // c["rpb"]) if c["rpb"] else 0
    return dict(ra=ra, ca=ca, lda=ca + c["pad"][0], rb=rb, cb=cb, ldb=cb + c["pad"][1], ldc=N + c["pad"][2], samples=samples,
                gate_ld=N + 8)


def workspace_floats(c):
    """what ops.gemm passes: its scratch when the call may need one, else none"""
    plain = not (c["bias"] or c["act"] or c["aux_out"] or c["gate"] or c["resid"] or c["rowadd"])
    return WS_FLOATS if (c["colsum"] or c["rowsum"] or (plain and c["K"] >= 2048)) else 0


def make_inputs(c):
    """name -> float64 CPU tensor of logical shape holding values of the storage format of that operand"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 12.0 - 6.0)
    M, N, K, dt = c["M"], c["N"], c["K"], c["dt"]
    Aop, Bop = r(M, K), r(K, N) / K ** 0.5
    if c["regime"] == "cancel":
        # the second half of K undoes the first but for a small remainder: |acc| << |A| |B|
        h = K // 2
        Aop[:, h:2 * h] = Aop[:, :h]
        Bop = rnd(Bop, dt)
        Bop[h:2 * h] = -Bop[:h] + rnd(r(h, N) * 2.0 ** -6 / K ** 0.5, dt)
    wide = c["regime"] == "wide"
    t = {"A": rnd(Aop if c["ak"] else Aop.t().contiguous(), dt), "B": rnd(Bop.t().contiguous() if c["bk"] else Bop, dt)}
    if c["bias"]:
        t["bias"] = rnd(uni(N) if wide else r(N), "f32")
    if c["act"] == 2:
        t["aux_in"] = rnd(uni(M, N) if wide else r(M, N), dt)
    if c["gate"]:
        t["gate"] = rnd(r(-(-M // c["rpb"]), N), "f32")
    if c["resid"]:
        t["resid"] = rnd(r(M, N), resid_dt(c))
    if c["rowadd"]:
        t["rowadd"] = rnd(r(c["rpb"], N), "f32")
    if c["beta"] != 0.0:
        t["C_old"] = rnd(r(M, N), "f32")
    if c["colsum"] == "out":
        t["colsum_old"] = rnd(r(N), "f32")
    if c["rowsum"]:
        t["rowsum_old"] = rnd(r(M), "f32")
    return t


def products(c, t, fault=None):
    """(acc, |A| |B|, op(A)) in float64: the expensive part, shared by every evaluation of a case"""
    Aop = t["A"] if c["ak"] else t["A"].t()
    Bop = t["B"].t() if c["bk"] else t["B"]
    return Aop @ Bop, Aop.abs() @ Bop.abs(), Aop, Bop


# ------------------------------------------------------------------------------------------------------------------------------
# reference, bound, simulated kernel
# ------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("drop_k_tile", "bias_shift8", "gate_prev_sample", "rowadd_div", "resid_row_down", "drop_beta", "alpha_after_bias",
          "colsum_last_row", "rowsum_one_split", "dgelu_unrounded")
FAULT_WITHIN_BOUND = ("dgelu_unrounded",)


def rounds_gradient(c):
    """parked-drain / warp-specialised GELU': the bf16 gradient is rounded before the multiply"""
    return c["target"]["variant"] in ("parked_drain", "warp_spec") and c["act"] == 2


def fault_applies(c, fault):
    """a fault needs the epilogue field it corrupts"""
    return {"drop_k_tile": True, "bias_shift8": bool(c["bias"]), "gate_prev_sample": bool(c["gate"]), "rowadd_div": bool(c["rowadd"]),
            "resid_row_down": bool(c["resid"]), "drop_beta": c["beta"] != 0.0, "alpha_after_bias": c["alpha"] != 1.0 and bool(c["bias"]),
            "colsum_last_row": bool(c["colsum"]), "rowsum_one_split": bool(c["rowsum"]), "dgelu_unrounded": rounds_gradient(c)}[fault]


def _rows(M, dev):
    return torch.arange(M, device=dev)


def evaluate(c, t, prod, stored=None, fault=None):
    """-> (ref, bound, sim).  ref / bound: name -> float64 reference value and error bound of every output of the case; sim: name ->
    that output as a kernel would store it (rounded at the stated points, with `fault` injected).  stored = the kernel's outputs:
    the reference continues from its aux_out, and takes the column sums from its C."""
    acc, absacc, Aop, Bop = prod
    M, N, K, dt = c["M"], c["N"], c["K"], c["dt"]
    dev, cb, u_act, u_out = acc.device, C_BOUND[c["dt"]], UNIT[c["dt"]], UNIT[out_dt(c)]
    alpha, beta = c["alpha"], c["beta"]
    ref, bound, sim = {}, {}, {}
    if fault == "drop_k_tile":
        k0 = max(0, K - 64)
        acc = acc - Aop[:, k0:] @ Bop[k0:]
    bias = t["bias"] if c["bias"] else torch.zeros(N, dtype=torch.float64, device=dev)
    if fault == "bias_shift8":
        bias = torch.roll(bias, -8)
    v = (acc + bias) * alpha if fault == "alpha_after_bias" else acc * alpha + bias
    E = K * U32 * abs(alpha) * absacc                 # carried accumulation error
    mag = abs(alpha) * absacc + bias.abs()            # the epilogue in absolute values
    R = torch.zeros_like(acc)                         # carried storage roundings
    if c["aux_out"]:
        ref["aux_out"], bound["aux_out"] = v, cb * (E + EPI_F32_OPS * U32 * mag) + u_act * v.abs()
        sim["aux_out"] = rnd(v, dt)
        v = stored["aux_out"] if stored is not None else sim["aux_out"]
        E, mag = torch.zeros_like(acc), v.abs()
    if c["act"] == 1:
        v = gelu(v)
        E = E * GELU_GRAD_SUP
    elif c["act"] == 2:
        gp = gelu_grad(t["aux_in"])
        if rounds_gradient(c):
            R = UNIT["bf16"] * v.abs() * gp.abs()
            if fault != "dgelu_unrounded" and stored is None:
                v = rnd(v, "bf16")
        v, E, mag = v * gp, E * gp.abs(), mag * GELU_GRAD_SUP
    m = _rows(M, dev)
    if c["gate"]:
        s = m // c["rpb"]
        if fault == "gate_prev_sample":
            s = torch.where((m % c["rpb"] == 0) & (m > 0), (m - 1) // c["rpb"], s)
        gt = t["gate"][s]
        v, E, mag, R = v * gt, E * gt.abs(), mag * gt.abs(), R * gt.abs()
    if c["resid"]:
        rr = t["resid"]
        if fault == "resid_row_down":          # the last 64-row tile reads the row below (the last row its own)
            idx = torch.where(m >= (M - 1) // 64 * 64, torch.clamp(m + 1, max=M - 1), m)
            rr = rr[idx]
        v, mag = v + rr, mag + rr.abs()
    if c["rowadd"]:
        idx = torch.clamp(m // c["rpb"], max=c["rpb"] - 1) if fault == "rowadd_div" else m % c["rpb"]
        ra = t["rowadd"][idx]
        v, mag = v + ra, mag + ra.abs()
    if beta != 0.0:
        mag = mag + (beta * t["C_old"]).abs()
        if fault != "drop_beta":
            v = v + beta * t["C_old"]
    ref["C"], bound["C"] = v, cb * (E + EPI_F32_OPS * U32 * mag) + R + u_out * v.abs()
    sim["C"] = rnd(v, out_dt(c))
    if c["colsum"]:
        Cs = stored["C"] if stored is not None else sim["C"]
        old = c["colsum_beta"] * t["colsum_old"] if c["colsum"] == "out" else torch.zeros(N, dtype=torch.float64, device=dev)
        ref["colsum"] = old + Cs.sum(0)
        bound["colsum"] = cb * (M + 2) * U32 * (old.abs() + Cs.abs().sum(0))
        keep = (M - 1) // 64 * 64 if fault == "colsum_last_row" else M
        sim["colsum"] = rnd(old + sim["C"][:keep].sum(0), "f32")
    if c["rowsum"]:
        old = c["rowsum_beta"] * t["rowsum_old"]
        ref["rowsum"] = old + Aop.sum(1)
        bound["rowsum"] = cb * (K + 2) * U32 * (old.abs() + Aop.abs().sum(1))
        keep = K // 2 if fault == "rowsum_one_split" else K
        sim["rowsum"] = rnd(old + Aop[:, :keep].sum(1), "f32")
    return ref, bound, sim


def reference(c, t, prod=None, stored=None):
    """name -> float64 reference of every output (C, aux_out, colsum, rowsum) and name -> its per-element bound"""
    ref, bound, _ = evaluate(c, t, prod if prod is not None else products(c, t), stored=stored)
    return ref, bound


def simulate(c, t, prod=None, fault=None):
    """the outputs a kernel would store: the reference rounded at the stated points, with one fault injected"""
    return evaluate(c, t, prod if prod is not None else products(c, t), fault=fault)[2]


def ratios(c, t, prod, got):
    """name -> worst err / bound over the elements of each output the case has (inf where an element with bound 0 is off)"""
    stored = {k: got[k] for k in ("aux_out", "C") if k in got}
    ref, bound = reference(c, t, prod, stored=stored)
    assert set(got) == set(ref), (c["name"], sorted(got), sorted(ref))
    out = {}
    for k, r in ref.items():
        err, b = (got[k] - r).abs(), bound[k]
        if not bool(torch.isfinite(got[k]).all()):
            out[k] = float("inf")
            continue
        q = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        out[k] = float(q.max())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the plan of a case
# ------------------------------------------------------------------------------------------------------------------------------
def plan_call(c, addr=None):
    """(positional arguments, keyword arguments) of ops.gemm_plan / the epilogue keywords of ops.gemm for the case.  addr: name ->
    device address (A, B, C, bias, aux_in, aux_out, gate, resid, rowadd, colsum_out, rowsum_a_out); None: aligned stand-ins with
    the case's 2-byte offsets."""
    g = geometry(c)
    if addr is None:
        addr = {k: (1 << 20) + (2 if (k in c["off"]) else 0) for k in ("A", "B", "C", "bias", "aux_in", "aux_out", "gate", "resid", "rowadd",
                                                                      "colsum_out", "rowsum_a_out")}
    dtc = 1 if c["dt"] == "bf16" else 0
    args = (dtc, c["ak"], c["bk"], c["M"], c["N"], c["K"], addr["A"], g["lda"], addr["B"], g["ldb"], addr["C"], g["ldc"])
    kw = dict(act=c["act"], alpha=c["alpha"], beta=c["beta"], out_f32=bool(c["out_f32"]), rows_per_batch=c["rpb"])
    if c["bias"]:
        kw["bias"] = addr["bias"]
    if c["act"] == 2:
        kw["aux_in"] = addr["aux_in"]
    if c["aux_out"]:
        kw["aux_out"] = addr["aux_out"]
    if c["gate"]:
        kw.update(gate=addr["gate"], gate_ld=g["gate_ld"])
    if c["resid"]:
        kw.update(resid=addr["resid"], resid_is_act=c["resid"] == "act")
    if c["rowadd"]:
        kw["rowadd"] = addr["rowadd"]
    if c["colsum"] == "out":
        kw.update(colsum_out=addr["colsum_out"], colsum_beta=c["colsum_beta"])
    if c["rowsum"]:
        kw.update(rowsum_a_out=addr["rowsum_a_out"], rowsum_a_beta=c["rowsum_beta"])
    return args, kw


def describe_plan(L, p):
    """the fields of a planned launch a case declares, as a target tuple"""
    name = L.GV_NAMES[p.variant]
    return (name, p.ntw or None, (p.mb, p.nb, p.stages) if name == "small_m" else None, P8[p.epi_kind] if p.epi_kind >= 0 else None,
            p.split > 1, ("GR_NONE", "GR_F32", "GR_BF16", "GR_F32_ROWSUM")[p.reduce], ("GS_NONE", "GS_FUSED", "GS_SEPARATE")[p.rowsum_mode],
            ("GC_NONE", "GC_FOLD", "GC_DEFERRED", "GC_SEPARATE")[p.colsum_mode], (p.xcd_parts > 0) if p.split > 1 else None)


def plan_of(c, L, ops, knobs="default", addr=None, workspace=None):
    """the launch vaw_gemm makes for the case: knobs "default" = default_gemm_knobs with the case's tile / generic switch (no GPU,
    no environment), None = the process's own (the debug switches must then be set by the caller)"""
    args, kw = plan_call(c, addr)
    if knobs == "default":
        knobs = ops.default_gemm_knobs(tile=c["tile"], force_generic=c["generic"])
    cap = -(-c["M"] // 64) if c["colsum"] == "partial" else None
    return ops.gemm_plan(*args, workspace_floats=workspace_floats(c) if workspace is None else workspace, knobs=knobs,
                         colsum_partial_rows=cap, **kw)

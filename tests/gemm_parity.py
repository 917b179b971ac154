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

vaw_gemm_fp8 (FP8_CASES, the second half of this file; test_gemm_fp8_parity_cpu.py and test_gpu_gemm_fp8.py) goes through the same
evaluate(): fp8 operand values, alpha times the two dequantisation scales on the accumulator, its own constant C_BOUND["fp8"], and
for the kinds that write C as fp8 bytes the outputs Cq (decoded bytes) and amax (the running max) next to C.

simulate() is the comparator's own test object: the reference rounded at the stated points ("kernel output" made on the CPU), with
one injected fault at a time (FAULTS)."""
import zlib

import torch

U32 = 2.0 ** -24
UNIT = {"bf16": 2.0 ** -8, "f32": U32, "e4m3": 2.0 ** -4, "e5m2": 2.0 ** -3}      # half an ulp, relative
C_BOUND = {"bf16": 1.0, "f32": 1.0, "fp8": 4.0}
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}                  # largest finite value
FMAX_BYTE = {"e4m3": 0x7E, "e5m2": 0x7B}                 # ... and its byte pattern
SUB_HALF = {"e4m3": 2.0 ** -10, "e5m2": 2.0 ** -17}      # half the smallest subnormal step
EPI_F32_OPS = 8
GELU_GRAD_SUP = 1.13              # sup |d/dx gelu_tanh(x)| = 1.1289 (x = 1.47)
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
WS_FLOATS = 1 << 26               # the grow-only scratch ops.gemm hands to vaw_gemm when the call may need one

# worst err / bound per variant on the MI355X, default process knobs, c = 1: (outputs stored as bf16, outputs stored as f32).  The
# bf16 figures sit just below 1 on every variant: the storage term is the exact half-ulp of bf16 rounding, and among a few thousand
# elements one always nearly attains it; the f32-stored outputs show the arithmetic's own share.
MEASURED = {"generic": (0.987, 0.686), "t128_bk32": (0.995, None), "t128_bk64": (0.988, 0.207), "ring256": (0.991, 0.209),
            "persistent": (0.991, 0.111), "small_m": (0.993, 0.212), "parked_drain": (0.986, 0.111), "warp_spec": (0.986, 0.111)}

# vaw_gemm_fp8 per epilogue kind, same run, c = C_BOUND["fp8"] = 4: (outputs stored as bf16, outputs stored as f32, fp8 bytes, running max).
# With c = 1 the f32-stored outputs gave 0.292 (K = 384), 0.339 (K = 256, cancelling products) and 2.067 (K = 128, 16 x 200), and
# the whole-tile K = 128 GELU' case 1.045 on a bf16 output: one v_mfma_scale_f32_16x16x128_f8f6f4 does not add its 128 products as an
# f32 chain.  It lines them up under the largest of them and cuts what lies about 13 bits below it (probe: 256 + 127 x 2^-6 comes
# back as 257.875 for 257.984, 256 + 127 x 2^-10 as 256; max |err| over a 16 x 200 output = 2^-12.6 of that largest product at
# K = 128), an error that does not grow with K while K u |A| |B| does -- so the shortest K is the worst case, and 4 is the next power
# of two above it.  Every injected fault is still caught with c = 4 (test_gemm_fp8_parity_cpu.py; the closest is 85 times the bound).
MEASURED_FP8 = {"P8_STORE": (0.981, 0.517, None, None), "P8_GELU": (0.982, None, None, None), "P8_GELU_Q": (0.982, None, 0.905, 0.037),
                "P8_DGELU": (0.955, None, None, None), "P8_DGELU_Q": (0.921, None, 0.878, 0.491), "P8_GATE": (0.950, 0.030, None, None),
                "wgrad_grouped": (None, 0.088, None, None)}

P8 = ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE", "P8_SLAB", "P8_ANY", "P8_WGRAD", "P8_RESID")
TARGET_FIELDS = ("variant", "ntw", "sm", "epi_kind", "split", "reduce", "rowsum_mode", "colsum_mode", "xcd")


def rnd(x, dt, saturate=True):
    """x (float64) rounded to the storage format, back in float64.  fp8: values beyond the largest finite one saturate (torch's own
    cast does not: 500.0 -> NaN as e4m3fn), unless saturate = False"""
    if dt in FMAX:
        if saturate:
            x = x.clamp(-FMAX[dt], FMAX[dt])
        return x.float().to(TORCH_DT[dt]).double()
    return x.to(TORCH_DT[dt]).double()


def fp8_bytes(x, dt):
    """fp8 values (float64) -> their byte patterns (uint8)"""
    return x.float().to(TORCH_DT[dt]).view(torch.uint8)


def fp8_decode(b, dt):
    """byte patterns (uint8) -> float64 values"""
    return b.view(TORCH_DT[dt]).double()


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
          "colsum_last_row", "rowsum_one_split", "dgelu_unrounded", "aux_in_row_down", "drop_scale_b", "a_decoded_as_e4m3",
          "q_scale_not_inverted", "q_unsaturated", "q_amax_unrounded")
FAULT_WITHIN_BOUND = ("dgelu_unrounded",)
FP8_FAULTS = ("drop_scale_b", "a_decoded_as_e4m3", "q_scale_not_inverted", "q_unsaturated", "q_amax_unrounded")      # need an fp8 case



def rounds_gradient(c):
    """parked-drain / warp-specialised GELU': the bf16 gradient is rounded before the multiply"""
    return c["target"].get("variant") in ("parked_drain", "warp_spec") and c["act"] == 2


def fault_applies(c, fault):
    """a fault needs the epilogue field it corrupts"""
    return {"drop_k_tile": True, "bias_shift8": bool(c["bias"]), "gate_prev_sample": bool(c["gate"]), "rowadd_div": bool(c["rowadd"]),
            "resid_row_down": bool(c["resid"]), "drop_beta": c["beta"] != 0.0, "alpha_after_bias": alpha_eff(c) != 1.0 and bool(c["bias"]),
            "colsum_last_row": bool(c["colsum"]), "rowsum_one_split": bool(c["rowsum"]), "dgelu_unrounded": rounds_gradient(c),
            "aux_in_row_down": c["act"] == 2, "drop_scale_b": "scale_b" in c, "a_decoded_as_e4m3": c.get("a_fmt") == "e5m2",
            "q_scale_not_inverted": bool(c.get("q_fmt")), "q_unsaturated": bool(c.get("q_fmt")), "q_amax_unrounded": bool(c.get("q_fmt"))}[fault]


def alpha_eff(c, drop_scale_b=False):
    """the factor on the accumulator, in float64: alpha, times the two f32 dequantisation scales of an fp8 case"""
    a = float(c["alpha"])
    if "scale_a" in c:
        a *= float(rnd(torch.tensor(c["scale_a"], dtype=torch.float64), "f32"))
        if not drop_scale_b:
            a *= float(rnd(torch.tensor(c["scale_b"], dtype=torch.float64), "f32"))
    return a


def _rows(M, dev):
    return torch.arange(M, device=dev)


def evaluate(c, t, prod, stored=None, fault=None):
    """-> (ref, bound, sim).  ref / bound: name -> float64 reference value and error bound of every output of the case; sim: name ->
    that output as a kernel would store it (rounded at the stated points, with `fault` injected).  stored = the kernel's outputs:
    the reference continues from its aux_out, and takes the column sums from its C."""
    acc, absacc, Aop, Bop = prod
    M, N, K, dt = c["M"], c["N"], c["K"], c["dt"]
    dev, cb, u_act, u_out = acc.device, C_BOUND[c.get("cb", c["dt"])], UNIT[c["dt"]], UNIT[out_dt(c)]
    alpha, beta = alpha_eff(c, drop_scale_b=fault == "drop_scale_b"), c["beta"]
    ref, bound, sim = {}, {}, {}
    if fault == "a_decoded_as_e4m3":       # the e5m2 bytes of A read as e4m3
        acc = fp8_decode(fp8_bytes(Aop.contiguous(), "e5m2"), "e4m3") @ Bop
    if fault == "drop_k_tile":
        k0 = max(0, K - c.get("ktile", 64))
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
        ai = t["aux_in"]
        if fault == "aux_in_row_down":         # the last 64-row tile reads the row below (the last row its own)
            mi = _rows(M, dev)
            ai = ai[torch.where(mi >= (M - 1) // 64 * 64, torch.clamp(mi + 1, max=M - 1), mi)]
        gp = gelu_grad(ai)
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
    if c.get("q_fmt"):
        # C leaves as fp8 bytes: r = bf16(v), q = fmt(clamp(r / scale)); the running max takes max |r|.  "C" stays an output of the
        # case: the bf16 tensor the bytes are made of (on the GPU the non-quantising twin launch writes it)
        qf, sc = c["q_fmt"], t["q_scale"]
        lim = FMAX[qf] * sc
        vc = v.clamp(-lim, lim)
        ref["Cq"], bound["Cq"] = vc, bound["C"] + UNIT[qf] * vc.abs() + SUB_HALF[qf] * sc
        lo, hi = (v.abs() - bound["C"]).max(), (v.abs() + bound["C"]).max()       # max |r| for any r within the bound of v
        ref["amax"], bound["amax"] = 0.5 * (lo + hi), 0.5 * (hi - lo)
        if stored is None:
            x = sim["C"] * sc if fault == "q_scale_not_inverted" else sim["C"] / sc
            sim["Cq"] = rnd(x, qf, saturate=fault != "q_unsaturated") * sc
            sim["amax"] = rnd(v.abs().max(), "f32") if fault == "q_amax_unrounded" else sim["C"].abs().max()
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
        if k == "Cq":          # an element certainly beyond the format's range must decode to exactly +-FMAX
            lim = FMAX[c["q_fmt"]] * t["q_scale"]
            sure = ref["C"].abs() - bound["C"] > lim
            if not bool((got[k][sure] == torch.sign(ref["C"][sure]) * lim).all()):
                out[k] = float("inf")
        if k == "amax" and float(rnd(got[k], "bf16")) != float(got[k]):       # the max of bf16 values is one of them
            out[k] = float("inf")
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


# ------------------------------------------------------------------------------------------------------------------------------
# vaw_gemm_fp8: A [M][K] values of a_fmt (e4m3 | e5m2), B [N][K] e4m3 values, both k-major; the same reference and bound with
#     alpha_eff = alpha * scale_a * scale_b   (float64 product of the f32 scales; neither a power of two, and not equal)
# on the accumulator (products of two fp8 values are exact in f32, so E = K u |alpha_eff| |A| |B| is the f32 accumulation alone),
# C_BOUND["fp8"], and K tiles of 128.  The *_Q kinds write C as fp8 bytes of q_fmt:
#     r = bf16(v), q = fmt(clamp(r / state[0], +-FMAX)), state[1] = max(state[1], max |r|)
#     Cq:   |decode(q) state[0] - clamp(v, +-FMAX state[0])| <= bound(C as bf16) + UNIT[fmt] |clamp(v)| + SUB_HALF[fmt] state[0];
#           an element with |v| - bound(C) > FMAX state[0] decodes to exactly +-FMAX; no NaN / Inf pattern
#     amax: within [max(|v| - bound(C)), max(|v| + bound(C))], and a bf16 value
# state[0] comes from the reference alone: the 0.99 quantile of |r| over FMAX (prepare_q), so about 1 % of the elements saturate.
# ------------------------------------------------------------------------------------------------------------------------------
FP8_SCALE_A = 0.3
FP8_TARGET_FIELDS = ("epi_kind", "a_fmt", "ntw", "rounds")
FP8_PAD = (16, 32, 8)
FP8_KINDS = {("P8_STORE", "e4m3"), ("P8_GELU", "e4m3"), ("P8_GELU_Q", "e4m3"), ("P8_DGELU", "e4m3"), ("P8_DGELU_Q", "e4m3"),
             ("P8_GATE", "e4m3"), ("P8_STORE", "e5m2"), ("P8_DGELU", "e5m2"), ("P8_DGELU_Q", "e5m2")}
F32OUT = dict(out_f32=1)
DGELU_PART = dict(act=2, colsum="partial")

# shapes: M-and-N edges (264 x 200: 8 live rows in the second row tile, 200 of 256 columns; 200 x 264: 72 live columns in the second
# 192-column tile), whole tiles with one K tile, the smallest admitted, and two launches of more than one item per workgroup on a
# grid of 16 (cus = 16: run under vaw_p8_set_reserved_cus)
E4, E3, W4, W3, S3, S4 = (264, 200, 256), (200, 264, 384), (256, 256, 128), (256, 192, 128), (16, 16, 128), (16, 200, 128)
# (name, shape, a_fmt, epilogue, extras, target = (epi_kind, a_fmt, ntw, rounds > 1))
_FP8_SPECS = [
    ("f8_store_e4_ntw4_bias_edge", E4, "e4m3", BIAS, {}, ("P8_STORE", "e4m3", 4, False)),
    ("f8_store_e4_ntw3_alpha_f32_edge", E3, "e4m3", dict(bias=1, alpha=0.25, out_f32=1), {}, ("P8_STORE", "e4m3", 3, False)),
    ("f8_store_e4_ntw4_cancel_f32", E4, "e4m3", F32OUT, dict(regime="cancel"), ("P8_STORE", "e4m3", 4, False)),
    ("f8_store_e4_ntw3_colsum_beta", W3, "e4m3", CS_OUT, {}, ("P8_STORE", "e4m3", 3, False)),
    ("f8_store_e4_ntw4_colsum_partial_edge", E4, "e4m3", CS_PART, {}, ("P8_STORE", "e4m3", 4, False)),
    ("f8_store_e4_ntw3_smallest", S3, "e4m3", BIAS, {}, ("P8_STORE", "e4m3", 3, False)),
    ("f8_store_e4_ntw4_smallest_f32", S4, "e4m3", F32OUT, {}, ("P8_STORE", "e4m3", 4, False)),
    ("f8_store_e4_ntw3_ld_padded", E3, "e4m3", BIAS, dict(pad=FP8_PAD), ("P8_STORE", "e4m3", 3, False)),
    ("f8_store_e5_ntw4_bias_edge", E4, "e5m2", BIAS, {}, ("P8_STORE", "e5m2", 4, False)),
    ("f8_store_e5_ntw3_colsum_partial_edge", E3, "e5m2", CS_PART, {}, ("P8_STORE", "e5m2", 3, False)),
    ("f8_gelu_ntw4_wide_edge", E4, "e4m3", GELU, dict(regime="wide"), ("P8_GELU", "e4m3", 4, False)),
    ("f8_gelu_ntw3_ld_padded_edge", E3, "e4m3", GELU, dict(pad=FP8_PAD), ("P8_GELU", "e4m3", 3, False)),
    ("f8_gelu_ntw4_whole", W4, "e4m3", GELU, {}, ("P8_GELU", "e4m3", 4, False)),
    ("f8_gelu_ntw3_rounds", (1288, 576, 256), "e4m3", GELU, dict(cus=16), ("P8_GELU", "e4m3", 3, True)),
    ("f8_geluq_ntw4_ld_padded_edge", E4, "e4m3", GELU, dict(q_fmt="e4m3", pad=FP8_PAD), ("P8_GELU_Q", "e4m3", 4, False)),
    ("f8_geluq_ntw3_edge", E3, "e4m3", GELU, dict(q_fmt="e4m3"), ("P8_GELU_Q", "e4m3", 3, False)),
    ("f8_geluq_ntw3_whole_e5m2_out", W3, "e4m3", GELU, dict(q_fmt="e5m2"), ("P8_GELU_Q", "e4m3", 3, False)),
    ("f8_dgelu_e4_ntw4_wide_edge", E4, "e4m3", DGELU, dict(regime="wide"), ("P8_DGELU", "e4m3", 4, False)),
    ("f8_dgelu_e4_ntw3_colsum_partial_edge", E3, "e4m3", DGELU_PART, {}, ("P8_DGELU", "e4m3", 3, False)),
    ("f8_dgelu_e4_ntw4_colsum_beta", W4, "e4m3", DGELU_CS, {}, ("P8_DGELU", "e4m3", 4, False)),
    ("f8_dgelu_e4_ntw4_rounds_colsum_partial", (1032, 1000, 256), "e4m3", DGELU_PART, dict(cus=16), ("P8_DGELU", "e4m3", 4, True)),
    ("f8_dgelu_e5_ntw4_colsum_partial_ld_padded_edge", E4, "e5m2", DGELU_PART, dict(pad=FP8_PAD), ("P8_DGELU", "e5m2", 4, False)),
    ("f8_dgelu_e5_ntw3_wide_edge", E3, "e5m2", DGELU, dict(regime="wide"), ("P8_DGELU", "e5m2", 3, False)),
    ("f8_dgeluq_e4_ntw4_edge", E4, "e4m3", DGELU, dict(q_fmt="e5m2"), ("P8_DGELU_Q", "e4m3", 4, False)),
    ("f8_dgeluq_e4_ntw3_colsum_beta_edge", E3, "e4m3", DGELU_CS, dict(q_fmt="e4m3"), ("P8_DGELU_Q", "e4m3", 3, False)),
    # the launch DiT's backward makes for fc2's input gradient: e5m2 dy, GELU', e5m2 bytes out, deferred column sums
    ("f8_dgeluq_e5_ntw4_colsum_partial_ld_padded_edge", E4, "e5m2", DGELU_PART, dict(q_fmt="e5m2", pad=FP8_PAD), ("P8_DGELU_Q", "e5m2", 4, False)),
    ("f8_dgeluq_e5_ntw3_edge", E3, "e5m2", DGELU, dict(q_fmt="e5m2"), ("P8_DGELU_Q", "e5m2", 3, False)),
    ("f8_gate_ntw4_rpb27_edge", E4, "e4m3", GATE27, {}, ("P8_GATE", "e4m3", 4, False)),
    ("f8_gate_ntw3_rpb24_ld_padded_edge", E3, "e4m3", GATE, dict(pad=FP8_PAD), ("P8_GATE", "e4m3", 3, False)),
]


def _build_fp8_cases():
    out = {}
    for name, (M, N, K), a_fmt, epi, kw, target in _FP8_SPECS:
        assert name not in out, name
        kw = dict(kw)
        extra = dict(a_fmt=a_fmt, q_fmt=kw.pop("q_fmt", None), cus=kw.pop("cus", 256), scale_a=FP8_SCALE_A, scale_b=1.7 / K ** 0.5,
                     cb="fp8", ktile=128)
        c = _c(name, -1, (1, 1), M, N, K, (None,) * len(TARGET_FIELDS), **kw, **epi)
        c.update(extra)
        c["target"] = dict(zip(FP8_TARGET_FIELDS, target))
        out[name] = c
    return out


FP8_CASES = _build_fp8_cases()


def is_edge(c):
    """live rows and live columns end inside a tile of the case's kernel"""
    return c["M"] % 256 != 0 and c["N"] % (64 * c["target"]["ntw"]) != 0 and c["M"] > 256 - 64 and c["N"] > 64


def make_fp8_inputs(c):
    """as make_inputs: name -> float64 CPU tensor; A holds values of a_fmt, B e4m3 values (about N(0, 1) both: scale_b carries the
    1 / sqrt(K)).  A *_Q case still needs prepare_q."""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 12.0 - 6.0)
    M, N, K = c["M"], c["N"], c["K"]
    A, B = rnd(r(M, K), c["a_fmt"]), rnd(r(N, K), "e4m3")
    if c["regime"] == "cancel":
        # the second half of K undoes the first but for one element in eight, which moves by a step or two of the format
        h = K // 2
        A[:, h:] = A[:, :h]
        nudge = (torch.rand(N, h, generator=g, dtype=torch.float64) < 0.125).double()
        B[:, h:] = rnd(-B[:, :h] * (1.0 + 0.125 * nudge), "e4m3")
    wide = c["regime"] == "wide"
    t = {"A": A, "B": B}
    if c["bias"]:
        t["bias"] = rnd(uni(N) if wide else r(N), "f32")
    if c["act"] == 2:
        t["aux_in"] = rnd(uni(M, N) if wide else r(M, N), "bf16")
    if c["gate"]:
        t["gate"] = rnd(r(-(-M // c["rpb"]), N), "f32")
    if c["resid"]:
        t["resid"] = rnd(r(M, N), "f32")
    if c["colsum"] == "out":
        t["colsum_old"] = rnd(r(N), "f32")
    return t


def prepare_q(c, t, prod):
    """A *_Q case's scale, from the reference alone: t["q_scale"] = f32(0.99 quantile of |bf16(v)| / FMAX) as a float64 0-dim tensor on
    the products' device.  -> the share of elements that saturate under it (the tests hold it between 0.1 % and 5 %)."""
    if not c["q_fmt"]:
        return None
    r = rnd(evaluate(dict(c, q_fmt=None), t, prod)[0]["C"], "bf16").abs().flatten()
    q99 = torch.sort(r).values[int(0.99 * (r.numel() - 1))]
    t["q_scale"] = rnd(q99 / FMAX[c["q_fmt"]], "f32")
    return float((r / t["q_scale"] > FMAX[c["q_fmt"]]).double().mean())


def fp8_plan_call(c, addr=None):
    """(positional arguments, keyword arguments) shared by ops.gemm_fp8_plan and ops.gemm_fp8 for the case.  addr: name -> device
    address; None: aligned stand-ins."""
    g = geometry(c)
    if addr is None:
        addr = {k: 1 << 20 for k in ("A", "B", "C", "scale_a", "scale_b", "bias", "aux_in", "aux_out", "gate", "resid", "colsum_out")}
    args = (c["M"], c["N"], c["K"], addr["A"], g["lda"], addr["scale_a"], addr["B"], g["ldb"], addr["scale_b"], addr["C"], g["ldc"])
    kw = dict(a_format=3 if c["a_fmt"] == "e5m2" else 2, act=c["act"], alpha=c["alpha"], out_f32=bool(c["out_f32"]), rows_per_batch=c["rpb"])
    if c["bias"]:
        kw["bias"] = addr["bias"]
    if c["act"] == 2:
        kw["aux_in"] = addr["aux_in"]
    if c["aux_out"]:
        kw["aux_out"] = addr["aux_out"]
    if c["gate"]:
        kw.update(gate=addr["gate"], gate_ld=g["gate_ld"], resid=addr["resid"])
    if c["colsum"] == "out":
        kw.update(colsum_out=addr["colsum_out"], colsum_beta=c["colsum_beta"])
    return args, kw


def fp8_plan_of(c, ops, cus=None, addr=None, workspace=None, q_state=1 << 20, part_rows=None, **kw_over):
    """the launch vaw_gemm_fp8 makes for the case.  cus = None: the case's own (256, or 16 for the multi-round cases), 0: the process's;
    part_rows: the capacity of the colsum_partial buffer when it is not the ceil(M / 128) rows the launch writes"""
    args, kw = fp8_plan_call(c, addr)
    kw.update(kw_over)
    cap = (-(-c["M"] // 128) if part_rows is None else part_rows) if c["colsum"] == "partial" else None
    ws = (WS_FLOATS if c["colsum"] == "out" else 0) if workspace is None else workspace
    return ops.gemm_fp8_plan(*args, workspace_floats=ws, cus=c["cus"] if cus is None else cus, colsum_partial_rows=cap,
                             out_fp8_state=q_state if c["q_fmt"] else 0, out_fp8_format=3 if c["q_fmt"] == "e5m2" else 2, **kw)


def describe_fp8_plan(L, p):
    """the fields of a planned fp8 launch a case declares, as a target tuple"""
    return (L.P8_NAMES[p.epi_kind], "e5m2" if p.a_e5m2 else "e4m3", p.ntw, p.tiles_m * p.tiles_n * p.split > p.grid)

"""Float64 reference, per-element error bound and case table for vaw_conv3x3 (imported by test_conv_parity_cpu.py, test_gpu_conv.py
and golden/make_conv_bits.py; no GPU needed, tensors live wherever the caller puts them).

Reference.  From the stored bf16 values: the patch matrix P [B H W][9 C] (columns (tap, channel), zero outside the image) written
with F.unfold in float64, the weight as Wm [Co][9 Ci], and the three modes as three products
    mode 0   y  [pixels][Co]  = P(x) Wm^T                 K = 9 Ci
    mode 1   dx [pixels][Ci]  = P(dy) Wflip               K = 9 Co     Wflip[(tap, co)][ci] = W[co][8 - tap][ci]
    mode 2   dW [Co][9 Ci]    = dy^T P(x)                 K = pixels
handed, with their absolute-value twins, to gemm_parity.evaluate(): the epilogue order (bias, residual in the act dtype or f32, beta,
column sums of the stored output, the bias gradient as the row sums of dy^T) and the bound are the statement the GEMM suite checks,
with c = C_BOUND["bf16"] = 1: the same MFMA instruction, the same f32 accumulators.

Regimes.  normal: Gaussian data against the bound.  int: small integers, every sum below 2^24 -- f32 outputs equal the reference,
bf16 outputs the reference rounded to bf16.  impulse: x (dy in modes 1 and 2) zero but for a single 1 at each corner, the middle of
each border and one interior pixel of every sample, weights tap + 9 ((ci + co) % 7): the output is the tap map itself, exactly.

simulate() is the comparator's own test object: the reference rounded at the stated points, with one injected fault (FAULTS).

Worst err / bound per kernel and mode on the MI355X (normal regime; pytest -m gpu tests/test_gpu_conv.py -s): MEASURED_CONV."""
import zlib

import torch
import torch.nn.functional as F

import gemm_parity as gp

WS_FLOATS = 1 << 26               # the grow-only scratch ops.conv3x3 hands to vaw_conv3x3
TARGET_FIELDS = ("variant", "ntw", "epi_kind", "split", "reduce", "bias_grad", "colsum_mode", "xcd")
DECLINE = "declined"              # the target of a case vaw_conv3x3 must leave to the explicit im2col + GEMM path (-3)

# worst err / bound on the MI355X, default process knobs, c = 1, normal regime: (kernel, mode) -> (bf16-stored outputs: y, dx;
# f32-stored outputs: dW, column sums, bias gradient).  The bf16 figures sit just below 1 as in MEASURED -- the storage term is the
# exact half-ulp of bf16 rounding; the f32 ones are far below it because K u |A| |B| grows with K (here the pixel count of mode 2, or
# the rows of a column sum) as a worst case while the kernels' f32 sums err like a random walk.  What that slack could hide in mode 2
# is what the int and impulse regimes are for: all 51 of their cases came back equal to the reference, element for element.
MEASURED_CONV = {("t128_bk64", 0): (0.951, 0.005), ("t128_bk64", 1): (0.953, 0.001), ("t128_bk64", 2): (None, 0.023),
                 ("persistent", 0): (0.967, None), ("persistent", 1): (0.950, None), ("persistent", 2): (None, 0.002)}


def _c(name, tile, mode, shape, Ci, Co, regime="normal", **epi):
    e = dict(bias=0, resid=None, beta=0.0, colsum=None, colsum_beta=0.0, rowsum=0, rowsum_beta=0.0)
    assert set(epi) <= set(e), (name, epi)
    e.update(epi)
    B, H, W = shape
    return dict(name=name, tile=tile, mode=mode, B=B, H=H, W=W, Ci=Ci, Co=Co, regime=regime, **e)


def _build_cases():
    out = {}

    def add(name, *a, **kw):
        assert name not in out, name
        out[name] = _c(name, *a, **kw)

    # ---- geometry: every shape in all three modes on both kernels.  192 / 64 channels: a ragged N tile of the 256-column kernel in
    # modes 0 and 2, whole tiles elsewhere; the regimes rotate so that each shape meets each of them
    geo = [(1, 2, 64), (2, 1, 64), (1, 2, 128), (1, 2, 96), (1, 4, 48), (4, 16, 5), (1, 64, 1), (64, 3, 3), (3, 16, 16)]
    # (the persistent kernel takes a weight gradient from two K splits of four 64-pixel tiles upward: the same images, more samples)
    geo_p8_m2 = [(4, 2, 64), (8, 1, 64), (2, 2, 128), (3, 2, 96), (3, 4, 48), (8, 16, 5), (8, 64, 1), (64, 3, 3), (3, 16, 16)]
    regimes = ("normal", "int", "impulse")
    for i, s in enumerate(geo):
        for mode in (0, 1, 2):
            for j, (kern, tile) in enumerate((("t128", 0), ("p8", 2 if (i + mode) % 2 else 3))):
                Ci, Co = (64, 192) if mode != 1 else (192, 64)
                sh = geo_p8_m2[i] if (mode == 2 and kern == "p8") else s
                add("geo_{}x{}x{}_m{}_{}".format(*sh, mode, kern), tile, mode, sh, Ci, Co, regime=regimes[(i + mode + j) % 3])
    # ---- ragged pixel counts: modes 0 and 1 stay on the 128 x 128 kernel under every switch value, mode 2 takes the explicit path
    for s in ((3, 5, 5), (1, 5, 7)):
        for tile in (-1, 0, 2, 3):
            for mode in (0, 1):
                add("ragged_{}x{}x{}_m{}_tile{}".format(*s, mode, tile), tile, mode, s, 64, 64, regime="int" if tile == 2 else "normal")
        add("ragged_{}x{}x{}_m2_declines".format(*s), -1, 2, s, 64, 64)
    # ---- channels
    s = (2, 8, 8)
    for Ci in (64, 128):
        for Co in (16, 64, 72, 200):
            tiles = (0,) if Co == 16 else (0, 3 if Co == 72 else 2)
            for tile in tiles:
                add(f"ch_m0_ci{Ci}_co{Co}_tile{tile}", tile, 0, s, Ci, Co)
                add(f"ch_m1_ci{Co}_co{Ci}_tile{tile}", tile, 1, s, Co, Ci)
    add("ch_m0_co16_under_tile2", 2, 0, s, 64, 16)
    add("ch_m1_ci16_under_tile2", 2, 1, s, 16, 64)
    for Ci in (8, 24, 64, 72):
        for Co in (16, 64, 72, 192):
            add(f"ch_m2_ci{Ci}_co{Co}_tile0", 0, 2, s, Ci, Co, regime="int" if (Ci, Co) == (24, 72) else "normal")
            tile = 2 if Ci == 72 else 3
            add(f"ch_m2_ci{Ci}_co{Co}_tile{tile}", tile, 2, (8, 8, 8), Ci, Co, regime="int" if (Ci, Co) == (8, 192) else "normal")
    add("ch_m0_ci24_declines", -1, 0, s, 24, 64)
    add("ch_m1_co24_declines", -1, 1, s, 64, 24)
    # ---- epilogues, mode 0
    for kern, tile in (("t128", 0), ("p8", 2), ("p8n3", 3)):
        add(f"epi_m0_none_{kern}", tile, 0, s, 64, 72)
        add(f"epi_m0_bias_{kern}", tile, 0, s, 64, 72, bias=1)
        add(f"epi_m0_bias_resid_{kern}", tile, 0, s, 64, 72, bias=1, resid="act")
    add("epi_m0_bias_resid_int_p8", 2, 0, (3, 8, 8), 64, 72, regime="int", bias=1, resid="act")
    add("epi_m0_resid_f32_t128", 0, 0, s, 64, 72, bias=1, resid="f32")
    add("epi_m0_resid_f32_under_tile2", 2, 0, s, 64, 72, resid="f32")
    add("epi_m0_colsum_t128", 0, 0, (3, 8, 8), 64, 72, bias=1, colsum="out", colsum_beta=0.5)
    add("epi_m0_colsum_under_tile2", 2, 0, (3, 8, 8), 64, 72, colsum="out", colsum_beta=0.5, regime="int")
    add("epi_m1_colsum_t128", 0, 1, (3, 8, 8), 72, 64, colsum="out", colsum_beta=0.5)
    # ---- epilogues, mode 2: beta, and the bias gradient once on each of its four ways (rowsum_a_beta 0 and 0.5)
    for beta in (0.0, 1.0, 0.5):
        add(f"epi_m2_beta{beta}_t128", 0, 2, s, 64, 72, beta=beta)
        add(f"epi_m2_beta{beta}_p8", 3, 2, (8, 8, 8), 64, 72, beta=beta, regime="int" if beta == 0.5 else "normal")
    add("bg_t128_split_reduce", 0, 2, (4, 16, 16), 64, 72, rowsum=1, rowsum_beta=0.5)
    add("bg_t128_split_reduce_int", 0, 2, (4, 16, 16), 24, 72, rowsum=1, regime="int")
    add("bg_t128_nosplit_fold", 0, 2, (1, 8, 8), 64, 72, rowsum=1, rowsum_beta=0.5, beta=0.5)
    add("bg_t128_nosplit_fold_int", 0, 2, (2, 8, 8), 24, 200, rowsum=1, regime="int")
    add("bg_p8_ntw3_fused", 3, 2, (2, 16, 16), 64, 72, rowsum=1, rowsum_beta=0.5, beta=1.0)
    add("bg_p8_ntw3_fused_int", 3, 2, (2, 16, 16), 24, 200, rowsum=1, regime="int")
    add("bg_p8_ntw4_separate", 2, 2, (2, 16, 16), 64, 72, rowsum=1, rowsum_beta=0.5)
    add("bg_p8_ntw4_separate_int", 2, 2, (2, 16, 16), 24, 264, rowsum=1, regime="int")
    # ---- splits, mode 2: 576 pixels = 9 K tiles, 5 + 4 on the persistent kernel; XCD-mapped, plain and no split on the 128 x 128
    add("split_p8_ragged_576", 2, 2, (1, 24, 24), 64, 72, beta=0.5)
    add("split_p8_ragged_576_ntw3", 3, 2, (1, 24, 24), 72, 200, regime="int")
    add("split_t128_xcd", 0, 2, (2, 16, 16), 64, 72)
    add("split_t128_plain3", 0, 2, (3, 16, 16), 64, 72, beta=1.0)
    add("split_t128_xcd_ragged", 0, 2, (1, 24, 24), 64, 72, regime="int")
    add("split_t128_none", 0, 2, (3, 8, 8), 64, 72)
    # ---- by shape (switch -1): the persistent kernel from half the CUs' worth of items, in every mode
    add("byshape_m0_p8", -1, 0, (8, 64, 64), 64, 192, bias=1, resid="act")
    add("byshape_m1_p8", -1, 1, (8, 64, 64), 192, 64)
    add("byshape_m2_p8", -1, 2, (8, 32, 32), 192, 192, rowsum=1)
    add("byshape_m0_t128", -1, 0, (2, 8, 8), 64, 192, bias=1)
    return out


CASES = _build_cases()

# The launch each case must reach (default knobs, 256 CUs), written out so that a change of the plan, or of a shape, that loses a
# kernel fails test_conv_parity_cpu.py instead of passing silently on another kernel.  DECLINE: vaw_conv3x3 returns -3.
#   (variant, ntw, epi_kind, split > 1, reduce, bias_grad, colsum_mode, XCD-mapped split)
_TARGETS = {
    "geo_1x2x64_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x64_m0_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x64_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x64_m1_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x64_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_4x2x64_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_2x1x64_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_2x1x64_m0_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_2x1x64_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_2x1x64_m1_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_2x1x64_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_8x1x64_m2_p8": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_1x2x128_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x128_m0_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x128_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x128_m1_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x128_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_2x2x128_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_1x2x96_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x96_m0_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x96_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x96_m1_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x2x96_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x2x96_m2_p8": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_1x4x48_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x4x48_m0_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x4x48_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x4x48_m1_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x4x48_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x4x48_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_4x16x5_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_4x16x5_m0_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_4x16x5_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_4x16x5_m1_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_4x16x5_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_8x16x5_m2_p8": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_1x64x1_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x64x1_m0_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x64x1_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x64x1_m1_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_1x64x1_m2_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_8x64x1_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_64x3x3_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_64x3x3_m0_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_64x3x3_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_64x3x3_m1_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_64x3x3_m2_t128": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "geo_64x3x3_m2_p8": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "geo_3x16x16_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x16x16_m0_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x16x16_m1_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x16x16_m1_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "geo_3x16x16_m2_t128": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', False),
    "geo_3x16x16_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ragged_3x5x5_m0_tile-1": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m1_tile-1": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m0_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m1_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m0_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m1_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m0_tile3": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m1_tile3": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_3x5x5_m2_declines": DECLINE,
    "ragged_1x5x7_m0_tile-1": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m1_tile-1": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m0_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m1_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m0_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m1_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m0_tile3": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m1_tile3": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ragged_1x5x7_m2_declines": DECLINE,
    "ch_m0_ci64_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci16_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci64_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co64_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci64_co64_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci72_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co72_tile3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci72_co64_tile3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co200_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci200_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci64_co200_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci200_co64_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci16_co128_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci64_co128_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co64_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci64_co128_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci72_co128_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co72_tile3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci72_co128_tile3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co200_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci200_co128_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_ci128_co200_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci200_co128_tile2": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m0_co16_under_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m1_ci16_under_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci8_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci8_co16_tile3": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "ch_m2_ci8_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci8_co64_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci8_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci8_co72_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci8_co192_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci8_co192_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci24_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci24_co16_tile3": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "ch_m2_ci24_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci24_co64_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci24_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci24_co72_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci24_co192_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci24_co192_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci64_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci64_co16_tile3": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "ch_m2_ci64_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci64_co64_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci64_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci64_co72_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci64_co192_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci64_co192_tile3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci72_co16_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci72_co16_tile2": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "ch_m2_ci72_co64_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci72_co64_tile2": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci72_co72_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci72_co72_tile2": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m2_ci72_co192_tile0": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "ch_m2_ci72_co192_tile2": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "ch_m0_ci24_declines": DECLINE,
    "ch_m1_co24_declines": DECLINE,
    "epi_m0_none_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_resid_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_none_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_p8": ('persistent', 4, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_resid_p8": ('persistent', 4, 'P8_RESID', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_none_p8n3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_p8n3": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_resid_p8n3": ('persistent', 3, 'P8_RESID', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_bias_resid_int_p8": ('persistent', 4, 'P8_RESID', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_resid_f32_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_resid_f32_under_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m0_colsum_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_FOLD', None),
    "epi_m0_colsum_under_tile2": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_FOLD', None),
    "epi_m1_colsum_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_FOLD', None),
    "epi_m2_beta0.0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m2_beta0.0_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "epi_m2_beta1.0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m2_beta1.0_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "epi_m2_beta0.5_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "epi_m2_beta0.5_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "bg_t128_split_reduce": ('t128_bk64', None, None, True, 'CVR_F32_ROWSUM', 'CVB_FUSED', 'GC_NONE', True),
    "bg_t128_split_reduce_int": ('t128_bk64', None, None, True, 'CVR_F32_ROWSUM', 'CVB_FUSED', 'GC_NONE', True),
    "bg_t128_nosplit_fold": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_FOLD', 'GC_NONE', None),
    "bg_t128_nosplit_fold_int": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_FOLD', 'GC_NONE', None),
    "bg_p8_ntw3_fused": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_FUSED', 'GC_NONE', False),
    "bg_p8_ntw3_fused_int": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_FUSED', 'GC_NONE', False),
    "bg_p8_ntw4_separate": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_SEPARATE', 'GC_NONE', False),
    "bg_p8_ntw4_separate_int": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_SEPARATE', 'GC_NONE', False),
    "split_p8_ragged_576": ('persistent', 4, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "split_p8_ragged_576_ntw3": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_NONE', 'GC_NONE', False),
    "split_t128_xcd": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "split_t128_plain3": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', False),
    "split_t128_xcd_ragged": ('t128_bk64', None, None, True, 'CVR_F32', 'CVB_NONE', 'GC_NONE', True),
    "split_t128_none": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "byshape_m0_p8": ('persistent', 3, 'P8_RESID', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "byshape_m1_p8": ('persistent', 3, 'P8_STORE', False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
    "byshape_m2_p8": ('persistent', 3, 'P8_SLAB', True, 'CVR_SLAB_T', 'CVB_FUSED', 'GC_NONE', False),
    "byshape_m0_t128": ('t128_bk64', None, None, False, 'CVR_NONE', 'CVB_NONE', 'GC_NONE', None),
}


def _attach_targets():
    for name, c in CASES.items():
        t = _TARGETS.get(name)
        c["target"] = t if t == DECLINE or t is None else dict(zip(TARGET_FIELDS, t))


# ------------------------------------------------------------------------------------------------------------------------------
# the GEMM each case is
# ------------------------------------------------------------------------------------------------------------------------------
def pixels(c):
    return c["B"] * c["H"] * c["W"]


def gemm_case(c):
    """the case as gemm_parity.evaluate() takes it: sizes of the mode's product and the epilogue fields"""
    Mp, Ci, Co = pixels(c), c["Ci"], c["Co"]
    M, N, K = ((Mp, Co, 9 * Ci), (Mp, Ci, 9 * Co), (Co, 9 * Ci, Mp))[c["mode"]]
    return dict(name=c["name"], M=M, N=N, K=K, dt="bf16", alpha=1.0, beta=c["beta"], bias=c["bias"], act=0, aux_out=0, gate=0,
                resid=c["resid"], rowadd=0, rpb=0, out_f32=1 if c["mode"] == 2 else 0, colsum=c["colsum"], colsum_beta=c["colsum_beta"],
                rowsum=c["rowsum"], rowsum_beta=c["rowsum_beta"], target={})


def out_dt(c):
    return "f32" if c["mode"] == 2 else "bf16"


def impulse_pixels(H, W):
    """(h, w) of the corners, the middle of each border and one interior pixel (the centre), without repeats"""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]
    return list(dict.fromkeys(pts))


def make_inputs(c):
    """name -> float64 CPU tensor holding values of the operand's storage format: x [pixels][Ci], dy [pixels][Co] (NHWC rows),
    w [Co][9 Ci] (the stored [Co][3][3][Ci]), bias [Co], resid [pixels][Co], C_old [Co][9 Ci], colsum_old, rowsum_old"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    B, H, W, Ci, Co, mode, Mp = c["B"], c["H"], c["W"], c["Ci"], c["Co"], c["mode"], pixels(c)
    exact = c["regime"] != "normal"
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    v = (lambda *s: ri(-2, 2, *s)) if exact else r
    t = {}
    Cact = Ci if mode == 0 else Co            # channels of the operand the taps gather from in modes 0 / 1
    if c["regime"] == "impulse":
        imp = torch.zeros(B, H, W, Cact, dtype=torch.float64)
        for b in range(B):
            for j, (h, w_) in enumerate(impulse_pixels(H, W)):
                imp[b, h, w_, (5 * j + b) % Cact] = 1.0
        imp = imp.view(Mp, Cact)
        tap = torch.arange(9, dtype=torch.float64).view(1, 9, 1)
        co, ci = torch.arange(Co).view(Co, 1, 1), torch.arange(Ci).view(1, 1, Ci)
        t["w"] = (tap + 9.0 * ((ci + co) % 7)).reshape(Co, 9 * Ci)
        if mode == 0:
            t["x"] = imp
        else:
            t["dy"] = imp
            if mode == 2:
                t["x"] = ri(-2, 2, Mp, Ci)
    else:
        if mode != 1:
            t["x"] = gp.rnd(v(Mp, Ci), "bf16")
        if mode != 0:
            t["dy"] = gp.rnd(v(Mp, Co), "bf16")
        if mode != 2:
            t["w"] = ri(-1, 1, Co, 9 * Ci) if exact else gp.rnd(r(Co, 9 * Ci) / (9 * (Ci if mode == 0 else Co)) ** 0.5, "bf16")
    if c["bias"]:
        t["bias"] = ri(-3, 3, Co) if exact else gp.rnd(r(Co), "f32")
    if c["resid"]:
        t["resid"] = ri(-2, 2, Mp, Co) if exact else gp.rnd(r(Mp, Co), "bf16" if c["resid"] == "act" else "f32")
    if c["beta"] != 0.0:
        t["C_old"] = ri(-4, 4, Co, 9 * Ci) if exact else gp.rnd(r(Co, 9 * Ci), "f32")
    if c["colsum"]:
        n = Co if mode == 0 else Ci
        t["colsum_old"] = ri(-4, 4, n) if exact else gp.rnd(r(n), "f32")
    if c["rowsum"]:
        t["rowsum_old"] = ri(-4, 4, Co) if exact else gp.rnd(r(Co), "f32")
    return t


def patches(c, a, fault=None):
    """a [pixels][C] -> P [pixels][9 C], P[m, tap * C + ch] = a[pixel(m) + offset(tap), ch], zero outside the image: F.unfold in
    float64.  The faults re-read masked taps from the flat tensor instead."""
    B, H, W = c["B"], c["H"], c["W"]
    C = a.shape[1]
    P = F.unfold(a.view(B, H, W, C).permute(0, 3, 1, 2), 3, padding=1).view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9, C)
    if fault in ("tap_lr_neighbour", "tap_ud_sample", "stale_mask"):
        Mp = B * H * W
        m = torch.arange(Mp, device=a.device)
        h, w_ = (m // W) % H, m % W
        hs, ws = ((m - 64) // W) % H, (m - 64) % W               # the pixel one K tile earlier (stale_mask: rows 64..127 of mode 2)
        flat = torch.cat([a, torch.zeros(1, C, dtype=a.dtype, device=a.device)])        # row Mp: what lies outside the tensor
        P = P.clone()
        for tap in range(9):
            dh, dw = tap // 3 - 1, tap % 3 - 1
            src = m + dh * W + dw
            raw = flat[torch.where((src >= 0) & (src < Mp), src, torch.full_like(src, Mp))]
            h_in, w_in = (h + dh >= 0) & (h + dh < H), (w_ + dw >= 0) & (w_ + dw < W)
            if fault == "tap_lr_neighbour":
                sel = h_in & ~w_in
            elif fault == "tap_ud_sample":
                sel = ~h_in & w_in
            else:
                stale_in = (hs + dh >= 0) & (hs + dh < H) & (ws + dw >= 0) & (ws + dw < W)
                rows = (m >= 64) & (m < 128)
                P[:, tap] = torch.where((rows & ~stale_in)[:, None], torch.zeros_like(raw), P[:, tap])
                sel = rows & stale_in & ~(h_in & w_in)
            P[:, tap] = torch.where(sel[:, None], raw, P[:, tap])
    return P.reshape(B * H * W, 9 * C)


def operands(c, t, fault=None):
    """(op(A), op(B)) of the mode's product, float64"""
    Ci, Co, mode = c["Ci"], c["Co"], c["mode"]
    if mode == 0:
        return patches(c, t["x"], fault), t["w"].t()
    if mode == 1:
        w3 = t["w"].view(Co, 9, Ci)
        if fault != "w_unflipped":
            w3 = w3.flip(1)
        return patches(c, t["dy"], fault), w3.permute(1, 0, 2).reshape(9 * Co, Ci)
    return t["dy"].t(), patches(c, t["x"], fault)


def products(c, t, fault=None):
    """(acc, |A| |B|, op(A), op(B)) in float64: the expensive part, shared by every evaluation of a case"""
    A, Bm = operands(c, t, fault)
    return A @ Bm, A.abs() @ Bm.abs(), A, Bm


# ------------------------------------------------------------------------------------------------------------------------------
# reference, bound, simulated kernel
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_FAULTS = {"bias_grad_one_split": "rowsum_one_split", "resid_row_down": "resid_row_down",
               "bias_shift8": "bias_shift8", "drop_beta": "drop_beta"}
FAULTS = ("drop_k_tile", "w_unflipped", "tap_lr_neighbour", "tap_ud_sample", "stale_mask", "slab_dropped", "bias_grad_one_split",
          "dw_transposed", "resid_row_down", "bias_shift8", "drop_beta")


def fault_applies(c, fault):
    """a fault needs the mode, geometry or epilogue field it corrupts"""
    if c["target"] == DECLINE:
        return False
    mode, Mp = c["mode"], pixels(c)
    return {"drop_k_tile": True, "w_unflipped": mode == 1, "tap_lr_neighbour": Mp > 1,
            "tap_ud_sample": c["B"] > 1,                                   # (one sample: such a tap reads outside the tensor)
            # (impulse: dy may be all zero on pixels 64..127, which hides what x was read there)
            "stale_mask": mode == 2 and Mp >= 128 and 64 % (c["H"] * c["W"]) != 0 and c["regime"] != "impulse",
            "slab_dropped": mode == 2 and bool(c["target"] and c["target"]["split"]), "bias_grad_one_split": bool(c["rowsum"]),
            "dw_transposed": mode == 2, "resid_row_down": bool(c["resid"]), "bias_shift8": bool(c["bias"]),
            "drop_beta": c["beta"] != 0.0}[fault]


def evaluate(c, t, prod, stored=None, fault=None):
    """-> (ref, bound, sim) as gemm_parity.evaluate(): name -> float64 reference, bound and simulated kernel output of C (y, dx or
    dW), colsum and rowsum (the bias gradient)"""
    gc = gemm_case(c)
    if fault in ("w_unflipped", "tap_lr_neighbour", "tap_ud_sample", "stale_mask"):
        prod = products(c, t, fault)
    elif fault == "drop_k_tile":           # modes 0 / 1: the first 64 channels of the centre tap (in the image at every pixel); mode 2: 64 pixels
        acc, absacc, A, Bm = prod
        k0 = gc["K"] - 64 if c["mode"] == 2 else 4 * (gc["K"] // 9)
        prod = (acc - A[:, k0:k0 + 64] @ Bm[k0:k0 + 64], absacc, A, Bm)
    elif fault == "slab_dropped":          # the first of two splits of K never reaches the output
        acc, absacc, A, Bm = prod
        k1 = (gc["K"] // 64 + 1) // 2 * 64
        prod = (acc - A[:, :k1] @ Bm[:k1], absacc, A, Bm)
    ref, bound, sim = gp.evaluate(gc, t, prod, stored=stored, fault=GEMM_FAULTS.get(fault))
    if fault == "dw_transposed":
        sim["C"] = sim["C"].t().contiguous().view(gc["M"], gc["N"])
    return ref, bound, sim


def simulate(c, t, prod, fault=None):
    return evaluate(c, t, prod, fault=fault)[2]


def ratios(c, t, prod, got):
    """name -> worst err / bound over the elements of each output (normal regime), or 0 / inf for equal / not equal to the reference
    rounded to the output's format (int and impulse regimes).  Every element counts; a NaN anywhere is inf."""
    stored = {"C": got["C"]}
    ref, bound, _ = evaluate(c, t, prod, stored=stored)
    assert set(got) == set(ref), (c["name"], sorted(got), sorted(ref))
    out = {}
    for k, r in ref.items():
        if got[k].shape != r.shape or not bool(torch.isfinite(got[k]).all()):
            out[k] = float("inf")
        elif c["regime"] == "normal":
            err, b = (got[k] - r).abs(), bound[k]
            q = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)),
                            torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            out[k] = float(q.max())
        else:
            out[k] = 0.0 if torch.equal(got[k], gp.rnd(r, out_dt(c) if k == "C" else "f32")) else float("inf")
    return out


def exact_regime_is_exact(c, t, prod):
    """int / impulse: every sum the kernel forms stays below 2^24, so that f32 accumulation in any order is exact"""
    acc, absacc = prod[0], prod[1]
    top = float(absacc.max()) + 64.0
    if c["colsum"]:
        top = max(top, float(acc.abs().sum(0).max()) * 1.01 + 64.0)
    if c["rowsum"]:
        top = max(top, float(prod[2].abs().sum(1).max()) + 64.0)
    return top < 2.0 ** 24


# ------------------------------------------------------------------------------------------------------------------------------
# the plan of a case
# ------------------------------------------------------------------------------------------------------------------------------
def plan_call(c, addr=None):
    """(positional arguments, keyword arguments) of ops.conv3x3 / ops.conv3x3_plan.  addr: name -> device address (act, act2, w, out,
    bias, resid, colsum_out, rowsum_a_out); None: aligned stand-ins"""
    if addr is None:
        addr = {k: 1 << 20 for k in ("act", "act2", "w", "out", "bias", "resid", "colsum_out", "rowsum_a_out")}
    mode = c["mode"]
    args = (1, mode, addr["act"], addr["act2"] if mode == 2 else None, None if mode == 2 else addr["w"], addr["out"], c["B"], c["H"], c["W"],
            c["Ci"], c["Co"])
    kw = dict(beta=c["beta"])
    if c["bias"]:
        kw["bias"] = addr["bias"]
    if c["resid"]:
        kw.update(resid=addr["resid"], resid_is_act=c["resid"] == "act")
    if c["colsum"]:
        kw.update(colsum_out=addr["colsum_out"], colsum_beta=c["colsum_beta"])
    if c["rowsum"]:
        kw.update(rowsum_a_out=addr["rowsum_a_out"], rowsum_a_beta=c["rowsum_beta"])
    return args, kw


def describe_plan(L, p):
    """the fields of a planned launch a case declares, as a target tuple; DECLINE for the explicit path"""
    if p.status == -3:
        return DECLINE
    return (L.GV_NAMES[p.variant], p.ntw or None, gp.P8[p.epi_kind] if p.epi_kind >= 0 else None, p.split > 1, L.CVR_NAMES[p.reduce],
            L.CVB_NAMES[p.bias_grad], ("GC_NONE", "GC_FOLD")[p.colsum_mode], (p.xcd_parts > 0) if p.split > 1 else None)


def plan_of(c, L, ops, knobs="default", addr=None, workspace=WS_FLOATS):
    """the launch vaw_conv3x3 makes for the case: knobs "default" = default_gemm_knobs (256 CUs) with the case's tile switch (no
    GPU, no environment), None = the process's own (the switch must then be set by the caller)"""
    args, kw = plan_call(c, addr)
    if knobs == "default":
        knobs = ops.default_gemm_knobs(tile=c["tile"])
    return ops.conv3x3_plan(*args, workspace_floats=workspace, knobs=knobs, check_status=False, **kw)


_attach_targets()

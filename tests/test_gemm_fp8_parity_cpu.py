"""The fp8 GEMM parity suite's own checks, without a GPU: every case of gemm_parity.FP8_CASES plans (vaw_gemm_fp8_plan, a stated CU
count) to the kernel instantiation it declares and the table as a whole reaches all 18 of them, both column-sum modes, an M-and-N
edge for every (kind, tile width), padded leading dimensions for every kind and a launch of more than one item per workgroup; the
comparator passes the reference rounded at the stated points and fails every applicable injected fault, the fp8-byte outputs
included; the plan's refusals carry the texts vaw_gemm_fp8 returns."""
import pytest
import torch

import gemm_parity as gp
from gemm_parity import FP8_CASES

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops

GC = ("GC_NONE", "GC_FOLD", "GC_DEFERRED")


@pytest.mark.parametrize("name", list(FP8_CASES))
def test_fp8_case_plans_to_its_declared_target(name):
    """256 CUs (16 for the two multi-round cases), the real leading dimensions, the workspace ops.gemm_fp8 passes"""
    c = FP8_CASES[name]
    p = gp.fp8_plan_of(c, ops)
    assert p.status == 0
    got = dict(zip(gp.FP8_TARGET_FIELDS, gp.describe_fp8_plan(L, p)))
    assert got == c["target"], (name, got, c["target"])
    M, N, K, bn = c["M"], c["N"], c["K"], 64 * p.ntw
    assert (p.tiles_m, p.tiles_n, p.nk, p.split, p.block) == (-(-M // 256), -(-N // bn), K // 128, 1, 512), name
    assert p.grid == min(p.tiles_m * p.tiles_n, c["cus"]) and p.lds_bytes == 2 * (4 + p.ntw) * 8192 + 32768
    assert (p.c_fp8, p.c_e5m2) == (int(bool(c["q_fmt"])), int(c["q_fmt"] == "e5m2"))
    mode = {None: "GC_NONE", "out": "GC_FOLD", "partial": "GC_DEFERRED"}[c["colsum"]]
    rows = -(-M // 128) if c["colsum"] else 0
    assert (GC[p.colsum_mode], p.colsum_rows, p.workspace_floats_used, p.launches) == \
        (mode, rows, rows * N if mode == "GC_FOLD" else 0, 2 if mode == "GC_FOLD" else 1), name
    if c["target"]["rounds"]:
        assert c["cus"] == 16 and p.grid == 16 and p.tiles_m * p.tiles_n > p.grid
    # the other tile width is another kernel: the plan, not the table, says which one a shape gets
    assert p.ntw == (4 if -(-N // 192) * 192 > -(-N // 256) * 256 else p.ntw)


def test_fp8_cases_reach_every_instantiation():
    seen = set()
    for c in FP8_CASES.values():
        t = c["target"]
        kind, fmt, ntw = t["epi_kind"], t["a_fmt"], t["ntw"]
        seen.add((kind, fmt, ntw))
        seen.add({None: "GC_NONE", "out": "GC_FOLD", "partial": "GC_DEFERRED"}[c["colsum"]])
        if gp.is_edge(c):
            seen.add(("edge", kind, ntw))
            if c["colsum"] == "partial":
                seen.add(("colsum_partial_edge", kind))
        if any(c["pad"]):
            assert c["pad"] == (16, 32, 8)
            seen.add(("pad", kind))
        if t["rounds"]:
            seen.add(("rounds", kind, bool(c["colsum"] == "partial")))
        if c["q_fmt"]:
            seen.add(("q_fmt", kind, c["q_fmt"]))
        if c["colsum"] in (None, "out"):
            seen.add(("colsum", kind, c["colsum"]))
        seen.add(("regime", c["regime"], kind, bool(c["out_f32"])))
        if c["M"] % 256 == 0 and c["N"] % (64 * ntw) == 0 and c["K"] == 128:
            seen.add(("whole_nk1", ntw))
        if c["M"] == 16:
            seen.add(("smallest", ntw))
    want = {(k, f, n) for (k, f) in gp.FP8_KINDS for n in (3, 4)}
    assert len(want) == 18 and want <= seen, sorted(map(str, want - seen))
    kinds = sorted({k for k, _ in gp.FP8_KINDS})
    want = {"GC_FOLD", "GC_DEFERRED"} | {("edge", k, n) for k in kinds for n in (3, 4)} | {("pad", k) for k in kinds}
    want |= {("rounds", "P8_GELU", False), ("rounds", "P8_DGELU", True)}
    want |= {("colsum_partial_edge", k) for k in ("P8_STORE", "P8_DGELU", "P8_DGELU_Q")}
    want |= {("colsum", k, m) for k in ("P8_DGELU", "P8_DGELU_Q") for m in (None, "out")} | {("colsum", "P8_STORE", "out")}
    want |= {("regime", "wide", "P8_GELU", False), ("regime", "wide", "P8_DGELU", False), ("regime", "cancel", "P8_STORE", True)}
    want |= {("q_fmt", k, f) for k in ("P8_GELU_Q", "P8_DGELU_Q") for f in ("e4m3", "e5m2")}
    want |= {("whole_nk1", 3), ("whole_nk1", 4), ("smallest", 3), ("smallest", 4)}
    assert want <= seen, sorted(map(str, want - seen))
    store = [c for c in FP8_CASES.values() if c["target"]["epi_kind"] == "P8_STORE"]
    assert any(c["bias"] and not c["out_f32"] for c in store) and any(c["bias"] and c["alpha"] == 0.25 and c["out_f32"] for c in store)
    assert any(c["colsum"] == "out" and c["colsum_beta"] == 0.5 for c in store)
    # a sample boundary inside a tile, and one inside a 4-row accumulator fragment; the gate's own row stride; an f32 residual
    gate = [c for c in FP8_CASES.values() if c["gate"]]
    assert {c["rpb"] for c in gate} == {24, 27} and all(c["resid"] == "f32" and gp.geometry(c)["gate_ld"] == c["N"] + 8 for c in gate)
    # scales that are no powers of two, and differ
    for c in FP8_CASES.values():
        for s in (c["scale_a"], c["scale_b"]):
            assert torch.frexp(torch.tensor(s, dtype=torch.float64))[0] != 0.5
        assert c["scale_a"] != c["scale_b"]


@pytest.fixture(scope="module")
def evaluated():
    """name -> (inputs, products, saturated share): made once, shared and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            c = FP8_CASES[name]
            t = gp.make_fp8_inputs(c)
            prod = gp.products(c, t)
            cache[name] = (t, prod, gp.prepare_q(c, t, prod))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(FP8_CASES))
def test_fp8_inputs_are_values_of_their_formats(name, evaluated):
    c = FP8_CASES[name]
    t = evaluated(name)[0]
    assert torch.equal(gp.rnd(t["A"], c["a_fmt"]), t["A"]) and torch.equal(gp.rnd(t["B"], "e4m3"), t["B"])
    assert torch.equal(gp.fp8_decode(gp.fp8_bytes(t["A"], c["a_fmt"]), c["a_fmt"]), t["A"])
    assert t["A"].shape == (c["M"], c["K"]) and t["B"].shape == (c["N"], c["K"])
    if c["regime"] == "cancel":
        acc, absacc = evaluated(name)[1][:2]
        assert float(acc.abs().mean()) < 0.1 * float(absacc.mean())


@pytest.mark.parametrize("name", list(FP8_CASES))
def test_fp8_comparator_passes_rounded_reference_and_fails_every_fault(name, evaluated):
    """as test_gemm_parity_cpu.py's, with the fp8 faults: a dropped scale_b, e5m2 bytes decoded as e4m3, GELU' reading the row below
    in the last 64-row tile, and for fp8 outputs a scale applied the wrong way round, a missing saturation and a running max taken
    before the bf16 rounding"""
    c = FP8_CASES[name]
    t, prod, share = evaluated(name)
    if c["q_fmt"]:
        assert 0.001 <= share <= 0.05, (name, share)
    clean = gp.ratios(c, t, prod, gp.simulate(c, t, prod))
    assert set(clean) == {"C"} | ({"aux_out"} if c["aux_out"] else set()) | ({"colsum"} if c["colsum"] else set()) | \
        ({"Cq", "amax"} if c["q_fmt"] else set())
    assert max(clean.values()) <= 1.0, (name, clean)
    for fault in gp.FAULTS:
        if not gp.fault_applies(c, fault):
            continue
        assert fault not in gp.FAULT_WITHIN_BOUND
        r = gp.ratios(c, t, prod, gp.simulate(c, t, prod, fault=fault))
        assert max(r.values()) > 1.0, (name, fault, r)
        if fault.startswith("q_"):      # caught on the byte path itself, not on the bf16 twin
            assert max(r["Cq"], r["amax"]) > 1.0 and r["C"] <= 1.0, (name, fault, r)


def test_every_fault_that_applies_to_fp8_is_exercised():
    applies = {f: sum(gp.fault_applies(c, f) for c in FP8_CASES.values()) for f in gp.FAULTS}
    for fault in gp.FP8_FAULTS + ("drop_k_tile", "bias_shift8", "gate_prev_sample", "resid_row_down", "alpha_after_bias", "colsum_last_row"):
        assert applies[fault] >= 2, (fault, applies)
    assert all(applies[f] == 0 for f in ("rowadd_div", "drop_beta", "rowsum_one_split", "dgelu_unrounded"))


def test_fp8_bound_constant_is_one_or_the_next_power_of_two():
    """C_BOUND["fp8"] may be raised to cover what the MFMA's own 128-wide sum does (and then only while the comparator test above
    still catches every fault with it)"""
    assert gp.C_BOUND["fp8"] >= 1.0 and float(torch.frexp(torch.tensor(gp.C_BOUND["fp8"]))[0]) == 0.5


def test_fp8_formats_round_as_stated():
    x = torch.tensor([500.0, -1e6, 448.0, 0.3, 2.0 ** -10, 2.0 ** -9], dtype=torch.float64)
    assert gp.rnd(x, "e4m3").tolist() == [448.0, -448.0, 448.0, 0.3125, 0.0, 2.0 ** -9]
    assert bool(torch.isnan(gp.rnd(x[:1], "e4m3", saturate=False)).all())
    assert gp.rnd(torch.tensor([1e9, 0.3, 2.0 ** -17], dtype=torch.float64), "e5m2").tolist() == [57344.0, 0.3125, 0.0]
    for fmt in ("e4m3", "e5m2"):
        b = torch.tensor([gp.FMAX_BYTE[fmt], gp.FMAX_BYTE[fmt] | 0x80, 1], dtype=torch.uint8)
        assert gp.fp8_decode(b, fmt).tolist() == [gp.FMAX[fmt], -gp.FMAX[fmt], 2 * gp.SUB_HALF[fmt]]
        # half an ulp, relative: the worst case sits just above a power of two
        v = torch.tensor([1.0 + 2 * gp.UNIT[fmt] * 0.999], dtype=torch.float64)
        assert abs(float(gp.rnd(v, fmt) - v)) <= gp.UNIT[fmt] * float(v)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals of the plan: the texts vaw_gemm_fp8 returns
# ------------------------------------------------------------------------------------------------------------------------------
A0 = 1 << 20
REFUSALS = {
    # name -> (M, N, K, lda, ldb, ldc, keywords of ops.gemm_fp8_plan, status, text)
    "K_not_128": (264, 200, 192, 192, 192, 200, {}, -1, "gemm_fp8: sizes (K % 128 == 0)"),
    "N_not_8": (264, 204, 256, 256, 256, 208, {}, -1, "gemm_fp8: leading dimensions"),
    "lda_not_16": (264, 200, 256, 264, 256, 200, {}, -1, "gemm_fp8: leading dimensions"),
    "e5m2_gelu": (264, 200, 256, 256, 256, 200, dict(a_format=L.BF8, bias=A0, act=1, aux_out=A0), -3,
                  "gemm_fp8: the forward epilogues (GELU, gated residual) take e4m3 activations"),
    "e5m2_gate": (264, 200, 256, 256, 256, 200, dict(a_format=L.BF8, bias=A0, aux_out=A0, gate=A0, gate_ld=208, resid=A0, rows_per_batch=24,
                                                       out_f32=True), -3,
                  "gemm_fp8: the forward epilogues (GELU, gated residual) take e4m3 activations"),
    "fp8_out_store": (264, 200, 256, 256, 256, 200, dict(bias=A0, out_fp8_state=A0), -1,
                      "gemm_fp8: fp8 output is offered for the GELU / GELU' epilogues (C then holds bytes, row stride ldc bytes)"),
    "fp8_out_f32": (264, 200, 256, 256, 256, 200, dict(act=2, aux_in=A0, out_f32=True, out_fp8_state=A0), -1,
                    "gemm_fp8: fp8 output is offered for the GELU / GELU' epilogues (C then holds bytes, row stride ldc bytes)"),
    "gelu_colsum": (264, 200, 256, 256, 256, 200, dict(bias=A0, act=1, aux_out=A0, colsum_out=A0, workspace_floats=1 << 20), -3,
                    "gemm_fp8: this epilogue combination has no fp8 kernel"),
    "partial_one_row_short": (264, 200, 256, 256, 256, 200, dict(act=2, aux_in=A0, colsum_partial_rows=2), -1,
                              "gemm_fp8: colsum_partial_out holds 2 rows, this launch writes 3"),
    "colsum_no_workspace": (264, 200, 256, 256, 256, 200, dict(colsum_out=A0), -1, "gemm_fp8: colsum_out needs a workspace"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_fp8_plan_refuses_with_the_calls_text(name):
    M, N, K, lda, ldb, ldc, kw, status, text = REFUSALS[name]
    args = (M, N, K, A0, lda, A0, A0, ldb, A0, A0, ldc)
    p = ops.gemm_fp8_plan(*args, cus=256, check_status=False, **kw)
    assert p.status == status and L.lib().vaw_last_error_string().decode() == text, (name, p.status, L.lib().vaw_last_error_string())
    with pytest.raises(vaw_amd.VawError) as ei:
        ops.gemm_fp8_plan(*args, cus=256, **kw)
    assert text in str(ei.value)


def test_fp8_plan_is_a_pure_function_of_a_stated_cu_count():
    """cus = 0 asks the process (256 without a device); a stated count decides alone"""
    a = (1288, 576, 256, A0, 256, A0, A0, 256, A0, A0, 576)
    p0, p256, p16 = (ops.gemm_fp8_plan(*a, cus=n) for n in (0, 256, 16))
    assert (p0.ntw, p0.grid) == (p256.ntw, p256.grid) == (3, 18) and (p16.ntw, p16.grid, p16.tiles_m * p16.tiles_n) == (3, 16, 18)
    # 192-column tiles only where they do not widen the padded output, then by rounds x 0.85
    for N, ntw in ((200, 4), (256, 4), (512, 4), (16, 3), (72, 3), (192, 3), (264, 3), (768, 3), (1152, 3)):
        assert ops.gemm_fp8_plan(264, N, 256, A0, 256, A0, A0, 256, A0, A0, N, cus=256).ntw == ntw, N

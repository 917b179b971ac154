"""The GEMM parity suite's own checks, without a GPU: every case of tests/gemm_parity.py plans to the kernel it declares and the
table as a whole reaches every launch choice of vaw_gemm_plan; the comparator passes "kernel output" made on the CPU (the float64
reference rounded at the stated points) and fails on every injected fault."""
import pytest
import torch

import gemm_parity as gp
from gemm_parity import CASES

from vaw_amd import _lib as L
from vaw_amd import ops


@pytest.mark.parametrize("name", list(CASES))
def test_case_plans_to_its_declared_target(name):
    """default knobs + the case's debug tile / generic switch, the real leading dimensions and alignments, the workspace ops.gemm passes"""
    c = CASES[name]
    p = gp.plan_of(c, L, ops)
    assert p.status == 0
    got = dict(zip(gp.TARGET_FIELDS, gp.describe_plan(L, p)))
    assert got == c["target"], (name, got, c["target"])
    assert p.workspace_floats_used <= gp.workspace_floats(c)
    if c["colsum"] == "partial":
        assert 1 <= p.colsum_rows <= -(-c["M"] // 64)


def test_cases_reach_every_target():
    """A table that lost a kernel, an epilogue kind, a tile shape, a reduce or a sum mode fails here."""
    seen = set()
    for c in CASES.values():
        t = c["target"]
        seen.add(t["variant"])
        seen.add(("layout", t["variant"], c["ak"], c["bk"]))
        if t["epi_kind"]:
            seen.add((t["variant"], t["epi_kind"], t["ntw"]))
        if t["sm"]:
            seen.add(("sm", t["sm"][:2]))
            seen.add(("stages", t["sm"][2]))
        seen.update({t["reduce"], t["rowsum_mode"], t["colsum_mode"]})
        if t["split"]:
            seen.add(("xcd", t["xcd"]))
            seen.add(("split", t["variant"]))
        for f in ("pad", "off"):
            if any(c[f]):
                seen.add((f, t["variant"]))
        if c["colsum"] == "out" and c["colsum_beta"] != 0.0:
            seen.add(("colsum_beta", t["variant"]))
        if c["colsum"] == "partial" and c["M"] % 256:
            seen.add(("colsum_partial_edge", t["variant"]))
        seen.add(("regime", c["regime"]))
        seen.add(("dt", c["dt"], t["variant"]))
    assert set(L.GV_NAMES) <= seen, seen
    want = {("persistent", k, n) for k in ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE", "P8_RESID", "P8_ANY", "P8_SLAB") for n in (3, 4)}
    want |= {(v, k, n) for v in ("parked_drain", "warp_spec") for k in ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE") for n in (3, 4)}
    want |= {("sm", s) for s in ((1, 1), (1, 2), (2, 2))} | {("stages", 3), ("stages", 4)}
    want |= {"GR_F32", "GR_BF16", "GR_F32_ROWSUM", "GS_FUSED", "GS_SEPARATE", "GC_FOLD", "GC_DEFERRED", "GC_SEPARATE"}
    want |= {("xcd", True), ("xcd", False)}
    want |= {("split", v) for v in ("t128_bk64", "ring256", "persistent", "generic")}
    # leading dimensions beyond the row on every MFMA variant the tile switch reaches, misaligned operands on the generic kernel
    want |= {("pad", v) for v in ("t128_bk64", "ring256", "persistent", "small_m", "parked_drain", "warp_spec", "generic")} | {("off", "generic")}
    want |= {("colsum_beta", v) for v in ("t128_bk64", "ring256", "persistent", "small_m", "parked_drain", "warp_spec", "generic")}
    want |= {("colsum_partial_edge", v) for v in ("t128_bk64", "ring256", "persistent", "small_m", "parked_drain")}
    want |= {("layout", v, 0, 1) for v in ("t128_bk64", "ring256", "persistent", "generic")}
    want |= {("layout", v, 0, 0) for v in ("t128_bk64", "ring256", "persistent", "generic")}
    want |= {("regime", r) for r in ("normal", "wide", "cancel")}
    want |= {("dt", "f32", "generic"), ("dt", "bf16", "generic")}
    assert want <= seen, sorted(map(str, want - seen))
    assert {c["off"] for c in CASES.values() if c["off"]} == {("A",), ("C",), ("aux_out",)}
    # a sample boundary inside a tile, and one inside a 4-row accumulator fragment
    assert any(c["gate"] and c["rpb"] % 8 == 0 and 64 % c["rpb"] for c in CASES.values())
    assert any(c["gate"] and c["rpb"] % 4 for c in CASES.values())


@pytest.fixture(scope="module")
def evaluated():
    """name -> (inputs, products): made once, shared by the comparator tests and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            t = gp.make_inputs(CASES[name])
            cache[name] = (t, gp.products(CASES[name], t))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_comparator_passes_rounded_reference_and_fails_every_fault(name, evaluated):
    """The reference rounded at the stated points is within the bound; each injected fault is beyond it on at least one output.
    A fault is skipped only on a case that lacks the epilogue field it corrupts (gemm_parity.fault_applies).  dgelu_unrounded --
    GELU' multiplied into the UNROUNDED input gradient where the parked-drain / warp-specialised kernels round it to bf16 first -- is
    the one fault expected to stay within the bound: the bound carries that rounding point, so both orders are accepted, and that
    is on record here."""
    c = CASES[name]
    t, prod = evaluated(name)
    clean = gp.ratios(c, t, prod, gp.simulate(c, t, prod))
    assert max(clean.values()) <= 1.0, (name, clean)
    for fault in gp.FAULTS:
        if not gp.fault_applies(c, fault):
            continue
        r = gp.ratios(c, t, prod, gp.simulate(c, t, prod, fault=fault))
        if fault in gp.FAULT_WITHIN_BOUND:
            assert max(r.values()) <= 1.0, (name, fault, r)
        else:
            assert max(r.values()) > 1.0, (name, fault, r)


def test_env_knob_subsets_plan_as_their_children_expect():
    """the subsets test_gpu_gemm.py runs under each environment knob, planned here with that knob set explicitly"""
    import test_gpu_gemm as tg
    assert set(tg.ENV_KNOBS) == set(tg.ENV_RUNS)
    for setting, (names, expect) in tg.ENV_RUNS.items():
        assert len(names) >= 3, setting
        for n in names:
            c = CASES[n]
            expect(c, gp.plan_of(c, L, ops, knobs=ops.default_gemm_knobs(tile=c["tile"], force_generic=c["generic"], **tg.ENV_KNOBS[setting])))


def test_every_fault_is_exercised():
    """(the faults of fp8 operands and outputs have their cases in gemm_parity.FP8_CASES)"""
    for fault in gp.FAULTS:
        pool = gp.FP8_CASES if fault in gp.FP8_FAULTS else CASES
        assert sum(gp.fault_applies(c, fault) for c in pool.values()) >= 2, fault


def test_reference_follows_the_header_order():
    """the reference against a second, literal statement of the header's formula on one small case with every field set"""
    c = gp._c("order", -1, (1, 1), 12, 8, 16, (None,) * len(gp.TARGET_FIELDS), dt="f32", bias=1, aux_out=1, act=1, gate=1, resid="f32",
              rpb=5, alpha=0.5, beta=0.25, colsum="out", colsum_beta=0.5)
    t = gp.make_inputs(c)
    ref, _ = gp.reference(c, t)
    pre = 0.5 * (t["A"] @ t["B"].t()) + t["bias"]
    torch.testing.assert_close(ref["aux_out"], pre, rtol=1e-14, atol=1e-14)
    aux = gp.rnd(pre, "f32")
    want = torch.nn.functional.gelu(aux, approximate="tanh") * t["gate"].repeat_interleave(5, 0)[:12] + t["resid"] + 0.25 * t["C_old"]
    torch.testing.assert_close(ref["C"], want, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ref["colsum"], 0.5 * t["colsum_old"] + gp.rnd(want, "f32").sum(0), rtol=1e-13, atol=1e-13)
    x = torch.linspace(-6, 6, 101, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
    torch.testing.assert_close(gp.gelu_grad(x.detach()), x.grad, rtol=1e-12, atol=1e-12)
    assert float(gp.gelu_grad(torch.linspace(-8, 8, 100001, dtype=torch.float64)).abs().max()) < gp.GELU_GRAD_SUP

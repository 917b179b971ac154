"""The conv3x3 parity suite's own checks, without a GPU: every case of tests/conv_parity.py plans to the kernel it declares and the
table as a whole reaches every launch choice of vaw_conv3x3_plan; the comparator passes "kernel output" made on the CPU (the
float64 reference rounded at the stated points) and fails on every injected fault; the reference agrees with F.conv2d and its
autograd gradients; every refusal of the plan has its row."""
import pytest
import torch
import torch.nn.functional as F

import conv_parity as cp
import gemm_parity as gp
from conv_parity import CASES, DECLINE

from vaw_amd import _lib as L
from vaw_amd import ops


@pytest.mark.parametrize("name", list(CASES))
def test_case_plans_to_its_declared_target(name):
    """default knobs (256 CUs) + the case's tile switch, aligned addresses, the workspace ops.conv3x3 passes"""
    c = CASES[name]
    p = cp.plan_of(c, L, ops)
    got = cp.describe_plan(L, p)
    if c["target"] == DECLINE:
        assert got == DECLINE and p.status == -3, (name, got, p.status)
        return
    assert p.status == 0, (name, p.status)
    assert dict(zip(cp.TARGET_FIELDS, got)) == c["target"], (name, got, c["target"])
    gc = cp.gemm_case(c)
    assert bool(p.transposed) == (got[0] == "persistent" and c["mode"] == 2)
    assert (p.M, p.N, p.K) == ((gc["N"], gc["M"], gc["K"]) if p.transposed else (gc["M"], gc["N"], gc["K"]))
    assert 0 < p.workspace_floats_used + 1 <= cp.WS_FLOATS and p.launches >= 1


def _seen():
    seen = set()
    for c in CASES.values():
        t = c["target"]
        if t == DECLINE:
            seen.add(("declined", c["mode"]))
            continue
        v, mode, W, H = t["variant"], c["mode"], c["W"], c["H"]
        M, N = cp.gemm_case(c)["M"], cp.gemm_case(c)["N"]
        if v == "persistent" and mode == 2:
            M, N = N, M
        seen.update({(v, mode), ("ntw", t["ntw"]), ("epi", t["epi_kind"]), t["reduce"], t["bias_grad"], t["colsum_mode"], ("regime", c["regime"], v, mode)})
        if t["split"]:
            seen.add(("xcd", t["xcd"]))
            if (cp.pixels(c) // 64) % 2:
                seen.add(("ragged_split", v))
        geo = "W|64" if 64 % W == 0 and W > 1 else "W>64" if W > 64 else "W=1" if W == 1 else "W coprime" if W % 2 else "W other"
        seen.add((geo, v, mode))
        if H == 1:
            seen.add(("H=1", v, mode))
        if H * W < 64:
            seen.add(("image < tile", v, mode))
        tm, tn = (256, 64 * t["ntw"]) if v == "persistent" else (128, 128)
        if M % tm:
            seen.add(("ragged M", v))
        if N % tn:
            seen.add(("ragged N", v))
        if N % 64:
            seen.add(("N off 64", v, mode))
        if c["resid"]:
            seen.add(("resid", c["resid"], v))
        if c["beta"] not in (0.0, 1.0):
            seen.add(("beta", v))
        if c["rowsum"]:
            seen.add(("rowsum_beta", c["rowsum_beta"] != 0.0, t["bias_grad"], t["reduce"]))
        if c["tile"] == -1:
            seen.add(("by shape", v, mode))
    return seen


def test_cases_reach_every_target():
    """A table that lost a kernel, a mode, a tile width, an epilogue kind, a reduce, a sum mode or a geometry fails here."""
    seen = _seen()
    kernels, modes = ("t128_bk64", "persistent"), (0, 1, 2)
    want = {(v, m) for v in kernels for m in modes} | {("ntw", 3), ("ntw", 4)}
    want |= {("epi", k) for k in ("P8_STORE", "P8_RESID", "P8_SLAB")}
    want |= {"CVR_NONE", "CVR_F32", "CVR_F32_ROWSUM", "CVR_SLAB_T", "CVB_NONE", "CVB_FUSED", "CVB_FOLD", "CVB_SEPARATE", "GC_NONE", "GC_FOLD"}
    want |= {("xcd", True), ("xcd", False), ("ragged_split", "persistent"), ("ragged_split", "t128_bk64")}
    want |= {(g, v, m) for g in ("W|64", "W>64", "W coprime", "W=1", "H=1", "image < tile") for v in kernels for m in modes}
    want |= {(r, v) for r in ("ragged M", "ragged N") for v in kernels}
    want |= {("N off 64", v, m) for v in kernels for m in modes}
    want |= {("resid", "act", v) for v in kernels} | {("resid", "f32", "t128_bk64")} | {("beta", v) for v in kernels}
    # the bias gradient on each of its four ways, with and without rowsum_a_beta
    want |= {("rowsum_beta", b, *w) for b in (True, False) for w in (("CVB_FUSED", "CVR_F32_ROWSUM"), ("CVB_FOLD", "CVR_NONE"),
                                                                    ("CVB_FUSED", "CVR_SLAB_T"), ("CVB_SEPARATE", "CVR_SLAB_T"))}
    want |= {("regime", r, v, m) for r in ("normal", "int", "impulse") for v in kernels for m in modes}
    want |= {("by shape", "persistent", m) for m in modes} | {("by shape", "t128_bk64", 0)} | {("declined", m) for m in modes}
    assert want <= seen, sorted(map(str, want - seen))
    # the statements of the issue about single cases
    for n, c in CASES.items():
        if n.startswith("ragged") and c["mode"] != 2:
            assert c["target"]["variant"] == "t128_bk64" and cp.pixels(c) % 64
        if c["target"] != DECLINE and (min(c["Ci"], c["Co"]) == 16 or (c["mode"] == 2 and c["Co"] < 64)) and "geo" not in n:
            assert c["target"]["variant"] == "t128_bk64", n
        if c["resid"] == "f32" or c["colsum"]:
            assert c["target"]["variant"] == "t128_bk64", n
    assert {c["tile"] for n, c in CASES.items() if n.startswith("ragged") and c["mode"] != 2} == {-1, 0, 2, 3}
    assert CASES["ch_m0_ci24_declines"]["target"] == DECLINE and CASES["ragged_3x5x5_m2_declines"]["target"] == DECLINE
    p = cp.plan_of(CASES["split_p8_ragged_576"], L, ops)
    assert (p.split, p.K // 64) == (2, 9)


@pytest.fixture(scope="module")
def evaluated():
    """name -> (inputs, products): made once, shared by the comparator tests and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            t = cp.make_inputs(CASES[name])
            cache[name] = (t, cp.products(CASES[name], t))
        return cache[name]
    return get


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["target"] != DECLINE])
def test_comparator_passes_rounded_reference_and_fails_every_fault(name, evaluated):
    """The reference rounded at the stated points passes (within the bound, or exactly in the int and impulse regimes, whose sums
    must all stay below 2^24); each injected fault fails on at least one output of every case it applies to."""
    c = CASES[name]
    t, prod = evaluated(name)
    if c["regime"] != "normal":
        assert cp.exact_regime_is_exact(c, t, prod), name
    clean = cp.ratios(c, t, prod, cp.simulate(c, t, prod))
    assert max(clean.values()) <= 1.0, (name, clean)
    for fault in cp.FAULTS:
        if cp.fault_applies(c, fault):
            r = cp.ratios(c, t, prod, cp.simulate(c, t, prod, fault=fault))
            assert max(r.values()) > 1.0, (name, fault, r)


def test_every_fault_is_exercised():
    for fault in cp.FAULTS:
        assert sum(cp.fault_applies(c, fault) for c in CASES.values()) >= 2, fault


def test_impulse_output_is_the_tap_map():
    """mode 0, one impulse in the interior: the 3 x 3 neighbourhood of the output holds tap + 9 ((ci + co) % 7), tap running
    against the offset (the pixel above-left of the impulse sees it through its bottom-right tap)"""
    c = CASES["geo_3x16x16_m0_t128"] if CASES["geo_3x16x16_m0_t128"]["regime"] == "impulse" else \
        next(c for c in CASES.values() if c["regime"] == "impulse" and c["mode"] == 0 and c["H"] >= 16 and c["W"] >= 16)
    t = cp.make_inputs(c)
    ref, _, _ = cp.evaluate(c, t, cp.products(c, t))
    H, W, Ci, Co = c["H"], c["W"], c["Ci"], c["Co"]
    j = cp.impulse_pixels(H, W).index((H // 2, W // 2))
    ci = (5 * j + 0) % Ci
    y = ref["C"].view(c["B"], H, W, Co)[0]
    for tap in range(9):
        dh, dw = tap // 3 - 1, tap % 3 - 1
        for co in (0, 5, Co - 1):
            assert float(y[H // 2 - dh, W // 2 - dw, co]) == tap + 9 * ((ci + co) % 7)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_agrees_with_conv2d_autograd(mode):
    """the three products against F.conv2d and its autograd gradients in float64, on one small case per mode (odd image, two samples)"""
    c = cp._c("conv2d", -1, mode, (2, 5, 7), 8, 16, bias=1 if mode == 0 else 0)
    c["target"] = None
    g = torch.Generator().manual_seed(mode)
    B, H, W, Ci, Co = 2, 5, 7, 8, 16
    x, dy = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64), torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    w, bias = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64), torch.randn(Co, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, bias, padding=1)
    (y * dy).sum().backward()
    nhwc = lambda a: a.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    t = {"x": nhwc(x), "dy": nhwc(dy), "w": w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci), "bias": bias}
    acc = cp.products(c, t)[0] + (bias if mode == 0 else 0.0)
    want = (nhwc(y.detach()), nhwc(xr.grad), wr.grad.permute(0, 2, 3, 1).reshape(Co, 9 * Ci))[mode]
    torch.testing.assert_close(acc, want, rtol=1e-12, atol=1e-12)
    if mode == 0:
        torch.testing.assert_close(cp.evaluate(c, t, cp.products(c, t))[0]["C"], want, rtol=1e-12, atol=1e-12)


A = 1 << 20
REFUSALS = [
    # (what, positional overrides, keywords) -> status and the text of vaw_last_error_string (None for -3: nothing is said)
    ("mode 3", dict(mode=3), {}, -1, "bad arguments"),
    ("no act", dict(act=0), {}, -1, "bad arguments"),
    ("no weight in mode 0", dict(w=0), {}, -1, "bad arguments"),
    ("no out", dict(out=0), {}, -1, "bad arguments"),
    ("W = 0", dict(W=0), {}, -1, "bad arguments"),
    ("beta on a bf16 output", {}, dict(beta=0.5), -1, "beta needs f32 output"),
    ("colsum_out without a workspace", {}, dict(colsum_out=A, workspace_floats=0), -1, "colsum_out needs a workspace"),
    ("colsum_out with a short workspace", {}, dict(colsum_out=A, workspace_floats=63), -1, "colsum_out needs a workspace"),
    ("bias gradient without a workspace", dict(mode=2, w=0, act2=A), dict(rowsum_a_out=A, workspace_floats=0), -1, "bias gradient needs a workspace"),
    # the two checks that used to depend on the shape: refused whether or not the persistent kernel would take the launch
    ("rowsum_a_out in mode 0, 128 x 128 shape", {}, dict(rowsum_a_out=A), -1, "belongs to mode 2"),
    ("rowsum_a_out in mode 0, persistent shape", dict(B=8, H=64, W=64, Co=192), dict(rowsum_a_out=A), -1, "belongs to mode 2"),
    ("rowsum_a_out in mode 1, forced persistent", dict(mode=1), dict(rowsum_a_out=A, tile=2), -1, "belongs to mode 2"),
    ("colsum_out in mode 2, 128 x 128 shape", dict(mode=2, w=0, act2=A), dict(colsum_out=A), -1, "not colsum_out"),
    ("colsum_out in mode 2, persistent shape", dict(mode=2, w=0, act2=A, B=8, H=32, W=32, Ci=192, Co=192), dict(colsum_out=A), -1, "not colsum_out"),
    ("f32", dict(dt=0), {}, -3, None),
    ("generic forced", {}, dict(force_generic=1), -3, None),
    ("mode 0, Ci = 24", dict(Ci=24), {}, -3, None),
    ("mode 1, Co = 24", dict(mode=1, Co=24), {}, -3, None),
    ("mode 2, Ci = 12", dict(mode=2, w=0, act2=A, Ci=12), {}, -3, None),
    ("mode 2, Co = 20", dict(mode=2, w=0, act2=A, Co=20), {}, -3, None),
    ("mode 2, 75 pixels", dict(mode=2, w=0, act2=A, B=3, H=5, W=5), {}, -3, None),
    ("mode 2 without x", dict(mode=2, w=0, act2=0), {}, -3, None),
    ("mode 0, Co = 20", dict(Co=20), {}, -3, None),
    ("mode 0, Co = 8", dict(Co=8), {}, -3, None),
    ("mode 0, 12 pixels", dict(B=1, H=3, W=4), {}, -3, None),
    ("mode 2, Co = 8", dict(mode=2, w=0, act2=A, Co=8), {}, -3, None),
    ("2^31 pixels", dict(B=1 << 15, H=256, W=256), {}, -3, None),
    ("act off by 2 bytes", dict(act=A + 2), {}, -3, None),
    ("out off by 8 bytes", dict(out=A + 8), {}, -3, None),
    ("bias off by 4 bytes", {}, dict(bias=A + 4), -3, None),
    ("resid off by 2 bytes", {}, dict(resid=A + 2), -3, None),
]


@pytest.mark.parametrize("what,pos,kw,status,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, pos, kw, status, text):
    """every -3 and every invalid-argument text of the plan; without the override the same call plans"""
    base = dict(dt=1, mode=0, act=A, act2=0, w=A, out=A, B=2, H=8, W=8, Ci=64, Co=64)
    order = ("dt", "mode", "act", "act2", "w", "out", "B", "H", "W", "Ci", "Co")

    def plan(pos, kw):
        kw = dict(kw)
        knobs = ops.default_gemm_knobs(tile=kw.pop("tile", -1), force_generic=kw.pop("force_generic", 0))
        a = dict(base, **pos)
        return ops.conv3x3_plan(*[a[k] for k in order], workspace_floats=kw.pop("workspace_floats", cp.WS_FLOATS), knobs=knobs,
                                check_status=False, **kw)
    assert plan(dict(mode=2, w=0, act2=A) if pos.get("mode") == 2 else {}, {}).status == 0
    p = plan(pos, kw)
    assert p.status == status, (what, p.status)
    if text:
        assert text in L.lib().vaw_last_error_string().decode(), (what, L.lib().vaw_last_error_string())

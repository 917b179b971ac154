"""The GroupNorm parity suite's own checks, without a GPU: every case of tests/gn_parity.py plans, in all four passes and under the
switch it names, to the launch it declares, and the table as a whole reaches every launch and edge it is there for; the comparator
passes "kernel output" made on the CPU (simulate(): the passes restated in f32 on the planned lanes and chunks) and flags every
injected fault on the cases named for it; in the exact regime the simulated kernels equal the reference, which is itself exactly
representable in f32; the closed form the propagated-statistics term differences is the autograd reference; and the three entry
points refuse null and misaligned pointers before any launch."""
import ctypes as C

import pytest
import torch

import gn_parity as gp
from gn_parity import CASES

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops


@pytest.mark.parametrize("name", list(CASES))
def test_case_plans_to_its_declared_target(name):
    c = CASES[name]
    for got in gp.plans_of(c, L, ops):
        assert got == c["target"], (name, got, c["target"])
    t = c["target"]
    assert t["nch"] == -(-c["HW"] // t["rows"]) and 1 <= t["last"] == c["HW"] - (t["nch"] - 1) * t["rows"] <= t["rows"], name
    assert (t["bg128"], t["bg256"]) == (c["B"] * c["G"] > 128, c["B"] * c["G"] > 256), name
    assert c["B"] * c["HW"] * c["C"] <= 2_200_000, name
    if c["dt"] == "bf16" and (c["C"] % 8 or c["C"] > 2048):
        assert t["variant"] == "quad", name               # the bf16 fallbacks, whatever the switch says


def _seen():
    seen = set()
    for c in CASES.values():
        t, cg = c["target"], c["C"] // c["G"]
        v = t["variant"]
        seen.update({(v, t["rows"]), (v, c["dt"]), (v, "regime", c["regime"]), (v, "film", c["film"]), (v, "silu", c["silu"]),
                     (v, "add", c["add"]), (v, "grad_beta", c["grad_beta"]), (v, "switch", c["switch"])})
        if v == "flat" and c["switch"] == -1:
            seen.add(("flat by shape", t["rows"]))
            if c["regime"] in ("normal", "exact"):
                seen.add(("flat by shape", t["rows"], c["regime"]))
        if gp.exact_bwd(c):
            seen.add((v, "exact backward"))
        if t["last"] == 1 and t["nch"] > 1:
            seen.add((v, "one-row last chunk"))
        if t["nch"] > 1:
            seen.add((v, "chunks"))
        if v == "flat":
            seen.add(("rpi", t["rpi"]))
            if c["HW"] < t["rpi"]:
                seen.add("fewer rows than row lanes")
            if t["nt"] <= 129:
                seen.add("half-dead workgroup")
            if 8 % cg and cg % 8:
                seen.add("group straddles an octet")
        else:
            if c["HW"] < 16:
                seen.add(("fewer rows than row groups", c["dt"]))
            if c["dt"] == "bf16" and c["C"] % 8:
                seen.add("bf16 C % 8 on quad")
            if c["dt"] == "bf16" and c["C"] > 2048:
                seen.add("bf16 C > 2048 on quad")
            if c["dt"] == "bf16" and c["C"] % 8 and c["switch"] == 1:
                seen.add("bf16 C % 8 on quad under switch 1")
            if 4 % cg and cg % 4:
                seen.add("group straddles a quad")
            if c["C"] > 64 and c["C"] % 64:
                seen.add("half-filled channel block")
        for k, ok in (("cg = 1", cg == 1), ("G = 1", c["G"] == 1), ("G = 64", c["G"] == 64), ("HW = 1", c["HW"] == 1), ("B > 16", c["B"] > 16),
                      ("B > 32", c["B"] > 32), ("B G > 128", t["bg128"]), ("B G > 256", t["bg256"]), ("C = 2048", c["C"] == 2048)):
            if ok:
                seen.add((v, k))
        if c["film"]:
            seen.add(("dfilm_ld != film_ld", gp.film_layout(c)[0] != gp.film_layout(c)[3]))
    return seen


def test_cases_reach_every_target():
    """A table that lost a launch, an edge or a flag combination fails here; every statement is made from the declared targets, which
    test_case_plans_to_its_declared_target holds to ops.gn_plan."""
    seen = _seen()
    assert len(set(CASES)) == len(CASES) and all(n == c["name"] for n, c in CASES.items())
    want = {("quad", 512), ("flat", 128), ("flat", 256), ("flat", 512), ("quad", "f32"), ("quad", "bf16"), ("flat", "bf16")}
    want |= {("flat by shape", r) for r in (128, 256, 512)} | {("flat by shape", r, g) for r in (256, 512) for g in ("normal", "exact")}
    for v in ("quad", "flat"):
        want |= {(v, "regime", r) for r in ("normal", "offset", "exact")} | {(v, "film", f) for f in (None, "3C", "2C8")}
        want |= {(v, "silu", s) for s in (True, False)} | {(v, "add", a) for a in (True, False)} | {(v, "grad_beta", g) for g in (0.0, 1.0, 0.5)}
        want |= {(v, "exact backward"), (v, "one-row last chunk"), (v, "chunks"), (v, "cg = 1"), (v, "G = 1"), (v, "B G > 128"), (v, "B G > 256")}
    want |= {("quad", "switch", s) for s in (-1, 0, 1)} | {("flat", "switch", s) for s in (-1, 1)}
    want |= {("rpi", 1), ("rpi", 256), ("rpi", 128), ("rpi", 85), ("rpi", 15), ("rpi", 32), "fewer rows than row lanes", "half-dead workgroup",
             "group straddles an octet", ("flat", "G = 64"), ("flat", "C = 2048"), ("quad", "C = 2048")}
    want |= {("fewer rows than row groups", "f32"), ("fewer rows than row groups", "bf16"), "bf16 C % 8 on quad", "bf16 C > 2048 on quad",
             "bf16 C % 8 on quad under switch 1", "group straddles a quad", "half-filled channel block", ("quad", "HW = 1"), ("quad", "B > 16"),
             ("quad", "B > 32"), ("flat", "B > 16"), ("dfilm_ld != film_ld", True)}
    assert want <= seen, sorted(map(str, want - seen))
    # the rows of the issue's tables, by name
    for name, fields in {"flat_512x16x8_g8_normal": (512, 1, 256, 256, 16), "flat_256x513x8_g2_normal": (512, 2, 256, 256, 1),
                         "flat_256x1024x8_g2_exact": (512, 2, 256, 256, 512), "flat_256x257x16_g4_normal": (256, 2, 256, 128, 1),
                         "flat_256x512x16_g4_exact": (256, 2, 256, 128, 256), "flat_128x385x24_g3_normal": (128, 4, 255, 85, 1),
                         "flatf_2x130x2048_g32_normal": (128, 2, 256, 1, 2), "flatf_2x40x1032_g24_normal": (128, 1, 129, 1, 40),
                         "flatf_3x129x136_g1_normal": (128, 2, 255, 15, 1), "flatf_3x129x136_g17_normal": (128, 2, 255, 15, 1),
                         "flatf_5x64x64_g64_normal": (128, 1, 256, 32, 64)}.items():
        t = CASES[name]["target"]
        assert (t["variant"], t["rows"], t["nch"], t["nt"], t["rpi"], t["last"]) == ("flat",) + fields, name
    assert CASES["flatf_5x64x64_g64_normal"]["target"]["bg256"] and gp.exact_bwd(CASES["flat_256x1024x8_g2_exact"])
    assert {(c["C"], c["G"]) for c in CASES.values() if c["switch"] == 1 and c["target"]["variant"] == "flat"} >= {(96, 32), (192, 32), (40, 10)}
    # the quad grid of the issue: every (C, G) meets every HW, and every B
    for Cc in (4, 12, 36, 68, 100):
        for G in {1, Cc // 4, Cc // 3 if Cc % 3 == 0 else 1, Cc}:
            if G <= 64:
                mine = [c for c in CASES.values() if (c["C"], c["G"]) == (Cc, G) and c["name"].startswith("quad")]
                assert {c["HW"] for c in mine} == {1, 3, 16, 513, 1040} and {c["dt"] for c in mine} == {"f32", "bf16"}, (Cc, G)
                assert {c["B"] for c in mine} >= {1, 17}, (Cc, G)
    assert {c["B"] for c in CASES.values() if c["name"].startswith("quad")} >= {1, 17, 33}
    for c in CASES.values():
        if c["regime"] == "exact":
            assert c["eps"] == 0.0 and not c["silu"], c["name"]
    assert gp.chain(CASES["flatf_2x130x2048_g32_normal"]) == 129 and gp.chain(CASES["quad_f32_17x1040x4_g1_offset"]) == 48


@pytest.fixture(scope="module")
def evaluated():
    """name -> (inputs, reference, bound): made once, shared and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            t = gp.make_inputs(CASES[name])
            cache[name] = (t,) + gp.evaluate(CASES[name], t)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_comparator_passes_the_simulated_kernels(name, evaluated):
    """simulate() without a fault is within every bound; in the exact regime it equals the reference, and the reference is exactly
    representable in f32 (the regime's premise, proved without the kernels); grad_beta 0 starts from NaN in dgamma and dbeta"""
    c = CASES[name]
    t, ref, bound = evaluated(name)
    r = gp.ratios(c, ref, bound, gp.simulate(c, t))
    assert max(r.values()) <= 1.0, (name, r)
    assert set(r) == set(gp.OUTPUTS if c["film"] else gp.OUTPUTS[:6])
    assert bool(torch.isnan(t["dgamma_old"]).all()) == (c["grad_beta"] == 0.0) == bool(torch.isnan(t["dbeta_old"]).all())
    if c["regime"] == "exact":
        ex = gp.exact_outputs(c)
        assert set(ex) >= {"mean", "rstd", "y"} and all(r[k] == 0.0 for k in ex if k in r), (name, r)
        assert gp.reference_fits_f32(c, ref), name
        G = c["G"]
        assert bool((ref["mean"] == ref["mean"].round()).all()) and bool(((1 / ref["rstd"]) == (1 / ref["rstd"]).round()).all())
        xg = t["x"].view(c["B"], c["HW"], G, -1)
        assert bool(((xg - ref["mean"][:, None, :, None]).sum((1, 3)) == 0).all()), name


@pytest.mark.parametrize("fault", list(gp.FAULTS))
def test_comparator_flags_every_fault(fault, evaluated):
    """each injected fault fails at least one output of each case named for it: on both mappings, against a bound and as an inequality"""
    names = gp.FAULT_CASES[fault]
    assert {CASES[n]["target"]["variant"] for n in names} == {"quad", "flat"}, fault
    for name in names:
        c = CASES[name]
        assert gp.fault_applies(c, fault), (fault, name)
        t, ref, bound = evaluated(name)
        r = gp.ratios(c, ref, bound, gp.simulate(c, t, fault=fault))
        assert max(r.values()) > 1.0, (fault, name, r)


def test_faults_are_named_and_exercised():
    assert set(gp.FAULT_CASES) == set(gp.FAULTS) and len(gp.FAULTS) >= 10
    for fault in gp.FAULTS:
        assert sum(gp.fault_applies(c, fault) for c in CASES.values()) >= 4, fault


@pytest.mark.parametrize("name", ["quad_f32_17x3x12_g3_offset", "flatf_2x33x192_g32_normal", "quad_bf16_17x16x36_g9_normal", "flatf_3x64x40_g10_exact"])
def test_closed_form_is_the_autograd_reference(name, evaluated):
    """what stat_term() differences: the kernels' formulas in float64 on the reference's statistics give the autograd gradients"""
    c = CASES[name]
    t, ref, _ = evaluated(name)
    cf = gp.closed_form(c, t, ref["mean"], ref["rstd"])
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)
    close(cf["y"], ref["y"])
    close(cf["dx"], ref["dx"])
    old = lambda k: c["grad_beta"] * t[k] if c["grad_beta"] != 0.0 else 0.0
    close(cf["A"].sum(0) + old("dgamma_old"), ref["dgamma"])
    close(cf["Bs"].sum(0) + old("dbeta_old"), ref["dbeta"])
    if c["film"]:
        close(cf["DS"], ref["dscale"])
        close(cf["DH"], ref["dshift"])


def test_measured_table_covers_every_mapping_pass_and_regime():
    keys = {(c["target"]["variant"] + "_" + c["dt"], p, c["regime"]) for c in CASES.values() for p in set(gp.PASS_OF.values())}
    assert set(gp.MEASURED_GN) == keys and all(0.0 <= v <= 1.0 for v in gp.MEASURED_GN.values())
    assert all(v == 0.0 for (m, p, r), v in gp.MEASURED_GN.items() if r == "exact" and p in ("stats", "fwd"))
    assert set(gp.PROPAGATED) <= set(gp.OUTPUTS[2:])


def test_reference_agrees_with_torch_group_norm():
    c = CASES["quad_f32_17x16x12_g4_offset"]
    t = gp.make_inputs(c)
    ref, _ = gp.reference(c, t)
    x = t["x"].permute(0, 2, 1)                                                        # [B][C][HW]
    y = torch.nn.functional.group_norm(x, c["G"], t["gamma"], t["beta"], eps=c["eps"])
    _, so, ho = gp.film_layout(c)[:3]
    y = y * (1 + t["emb"][:, so:so + c["C"], None]) + t["emb"][:, ho:ho + c["C"], None]
    torch.testing.assert_close(ref["y"], torch.nn.functional.silu(y).permute(0, 2, 1), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# host checks of the three entry points: refused with VAW_ERR_INVALID and the entry point's name, before any launch (no GPU here)
# ------------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_entry_points_refuse_null_and_misaligned_pointers():
    lib = vaw_amd.lib()
    keep, a = _aligned(256)

    def refused(rc, prefix):
        assert rc == -1
        assert lib.vaw_last_error_string().decode().startswith(prefix), lib.vaw_last_error_string()

    def calls(dt, B, HW, Cc, G):
        """entry point -> (argument list of a call that passes every host check, {argument index: name} of its pointers)"""
        fwd = [dt, a, a, a, a, a, 3 * Cc, 1, a, a, a, B, HW, Cc, G, 1e-5, a, None]
        app = [dt, a, a, a, a, a, a, a, 3 * Cc, 1, a, B, HW, Cc, G, None]
        bwd = [dt, a, a, a, a, a, a, a, a, 3 * Cc, 1, a, a, a, a, 1.0, a, a, 3 * Cc, B, HW, Cc, G, a, None]
        return {"groupnorm_fwd": (lib.vaw_groupnorm_fwd, fwd, dict(x=1, gamma=2, beta=3, scale=4, shift=5, y=8, mean=9, rstd=10, workspace=16)),
                "groupnorm_apply": (lib.vaw_groupnorm_apply, app, dict(x=1, mean=2, rstd=3, gamma=4, beta=5, scale=6, shift=7, y=10)),
                "groupnorm_bwd": (lib.vaw_groupnorm_bwd, bwd, dict(dout=1, x=2, mean=3, rstd=4, gamma=5, beta=6, scale=7, shift=8, dx_add=11, dx=12,
                                                                   dgamma=13, dbeta=14, dscale=16, dshift=17, workspace=23))}

    def call(fn, args, at, change):
        """the call with one argument changed: every call made here carries exactly one defect, so none reaches a launch"""
        return fn(*[change(v) if i == at else v for i, v in enumerate(args)])

    try:
        # (dtype, switch, sizes, the alignment of the activations under the launch the plan picks)
        for dt, switch, size, act in ((L.F32, -1, (2, 16, 32, 32), 16), (L.BF16, -1, (2, 16, 32, 32), 8), (L.BF16, 1, (2, 16, 32, 32), 16),
                                      (L.BF16, 1, (2, 16, 36, 9), 8), (L.BF16, -1, (512, 16, 8, 8), 16)):
            lib.vaw_debug_gn_flat(switch)
            assert ops.gn_plan(L.GN_APPLY, dt, *size).variant == (L.GNV_FLAT if (dt, act) == (L.BF16, 16) else L.GNV_QUAD)
            for who, (fn, args, ptrs) in calls(dt, *size).items():
                acts = [k for k in ("x", "y", "dout", "dx", "dx_add") if k in ptrs]
                required = [k for k in ptrs if k not in ("scale", "shift", "dx_add", "dscale", "dshift")]
                for k in required:
                    refused(call(fn, args, ptrs[k], lambda v: None), who + ":")
                for k in acts:                                                 # one element off, and half the alignment off
                    for off in {4 if dt == L.F32 else 2, act // 2}:
                        refused(call(fn, args, ptrs[k], lambda v: v + off), who + ":")
                        assert "aligned" in lib.vaw_last_error_string().decode(), (who, k, off)
                for k in ("gamma", "beta", "scale", "shift"):
                    for off in (4, 8):
                        refused(call(fn, args, ptrs[k], lambda v: v + off), who + ":")
                        assert "aligned" in lib.vaw_last_error_string().decode(), (who, k, off)
                refused(call(fn, args, ptrs["shift"], lambda v: None), who + ":")          # scale without shift
                refused(call(fn, args, ptrs["scale"], lambda v: None), who + ":")          # shift without scale
                if who == "groupnorm_bwd":                                                 # FiLM without its gradient rows
                    refused(call(fn, args, ptrs["dscale"], lambda v: None), who + ":")
                    refused(call(fn, args, ptrs["dshift"], lambda v: None), who + ":")
    finally:
        lib.vaw_debug_gn_flat(-1)
    del keep

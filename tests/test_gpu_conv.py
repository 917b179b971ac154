"""vaw_conv3x3 against the float64 reference of tests/conv_parity.py on every kernel, mode, epilogue and edge the case table names:
each case sets its tile switch, asks vaw_conv3x3_plan (the process's own knobs, the real addresses) for the call it is about to make
and refuses to run on any other kernel, launches through ops.conv3x3, compares every element of every output against the bound (or
exactly, in the int and impulse regimes), and runs twice for bitwise-equal results.  The gathered inputs sit between NaN guards of
(W + 2) * C elements, so a tap that is not masked poisons the output; the outputs sit between canaries; the workspace starts as NaN.
ops.fallbacks moves on the cases that plan to the explicit path, and on no other."""
import warnings

import pytest
import torch

import conv_parity as cp
import gemm_parity as gp
from conv_parity import CASES, DECLINE

pytestmark = pytest.mark.gpu

from vaw_amd import _lib as L
from vaw_amd import ops

DEV = "cuda"
OUT_CANARY = 768.0        # exact in bf16
GUARD = 64                # canary elements in front of and behind every output
TDT = gp.TORCH_DT


def _guarded(values, dt, guard, fill):
    """values [R][C] (float64) in the middle of a flat buffer with `guard` elements of `fill` on both sides -> (flat, address)"""
    n = values.numel()
    flat = torch.full((n + 2 * guard,), fill, dtype=TDT[dt], device=DEV)
    flat[guard:guard + n] = values.reshape(-1).to(TDT[dt])
    return flat, flat.data_ptr() + guard * flat.element_size()


class _Run:
    """one launch of a case on fresh output buffers"""

    def __init__(self, c, t):
        gc = cp.gemm_case(c)
        mode, W, Ci, Co = c["mode"], c["W"], c["Ci"], c["Co"]
        self.c, self.keep, self.addr, self.outs = c, [], {}, {}
        nan = float("nan")

        def inp(name, values, dt, guard, fill=nan):
            flat, a = _guarded(values, dt, guard, fill)
            self.keep.append(flat)
            self.addr[name] = a

        if mode == 0:
            inp("act", t["x"], "bf16", (W + 2) * Ci)
        else:
            inp("act", t["dy"], "bf16", (W + 2) * Co)
        if mode == 2:
            inp("act2", t["x"], "bf16", (W + 2) * Ci)
        else:
            inp("w", t["w"], "bf16", (W + 2) * Ci)
        if c["bias"]:
            inp("bias", t["bias"], "f32", GUARD)
        if c["resid"]:
            inp("resid", t["resid"], "bf16" if c["resid"] == "act" else "f32", GUARD)

        def out(name, key, R, Cc, dt, init=None):
            vals = init if init is not None else torch.full((R, Cc), OUT_CANARY, dtype=torch.float64)
            flat, a = _guarded(vals, dt, GUARD, OUT_CANARY)
            self.addr[name] = a
            self.outs[key] = (flat, flat.clone(), R, Cc)

        out("out", "C", gc["M"], gc["N"], cp.out_dt(c), t.get("C_old"))
        if c["colsum"]:
            out("colsum_out", "colsum", 1, gc["N"], "f32", t["colsum_old"][None])
        if c["rowsum"]:
            out("rowsum_a_out", "rowsum", 1, gc["M"], "f32", t["rowsum_old"][None])

    def plan(self):
        ws = ops.scratch_f32(torch.device(DEV, torch.cuda.current_device()), 0)
        return cp.plan_of(self.c, L, ops, knobs=None, addr=self.addr, workspace=ws.numel()), ws

    def launch(self):
        args, kw = cp.plan_call(self.c, self.addr)
        ran = ops.conv3x3(*args, **kw)
        torch.cuda.synchronize()
        return ran

    def results(self):
        """name -> float64 output; the canaries around every output are checked on the way"""
        got = {}
        for key, (flat, init, R, Cc) in self.outs.items():
            n = R * Cc
            assert torch.equal(flat[:GUARD], init[:GUARD]) and torch.equal(flat[GUARD + n:], init[GUARD + n:]), \
                (self.c["name"], key, "canaries next to the output were written")
            v = flat[GUARD:GUARD + n].view(R, Cc).double()
            got[key] = v[0] if key in ("colsum", "rowsum") else v
        return got

    def raw(self):
        return [o[0] for o in self.outs.values()]


def run_case(c):
    """-> name -> worst err / bound of each output of the case (asserted <= 1); {} for a case that must decline"""
    t = cp.make_inputs(c)
    L.lib().vaw_debug_gemm_tile(c["tile"])
    try:
        a, b = _Run(c, t), _Run(c, t)
        p, ws = a.plan()
        before = dict(ops.fallbacks)
        if c["target"] == DECLINE:
            assert p.status == -3, (c["name"], p.status)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                assert a.launch() is False
            key = ("conv3x3", ("fwd", "dgrad", "wgrad")[c["mode"]], c["B"], c["H"], c["W"], c["Ci"], c["Co"])
            assert ops.fallbacks.get(key, 0) == before.get(key, 0) + 1 and {k: v for k, v in ops.fallbacks.items() if k != key} == \
                {k: v for k, v in before.items() if k != key}, (c["name"], "ops.fallbacks")
            for flat, init, _, _ in a.outs.values():
                assert torch.equal(flat, init), (c["name"], "a declined call wrote its output")
            return {}
        assert p.status == 0, (c["name"], p.status)
        got_t = dict(zip(cp.TARGET_FIELDS, cp.describe_plan(L, p)))
        assert got_t == c["target"], (c["name"], got_t, c["target"])
        assert p.workspace_floats_used <= ws.numel()
        ws.fill_(float("nan"))
        assert a.launch() is True
        ws.fill_(float("nan"))
        assert b.launch() is True
        assert ops.fallbacks == before, (c["name"], "ops.fallbacks moved on a case the kernels take")
        got = a.results()
        b.results()
        for x, y in zip(a.raw(), b.raw()):        # fixed-order reductions: a repeat is bitwise equal
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (c["name"], "a second launch gave other bits")
    finally:
        L.lib().vaw_debug_gemm_tile(-1)
    td = {k: v.to(DEV) for k, v in t.items()}
    ratios = cp.ratios(c, td, cp.products(c, td), got)
    print(c["name"], c["target"]["variant"], "mode", c["mode"], c["regime"], {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (c["name"], ratios)
    return ratios


@pytest.mark.parametrize("name", list(CASES))
def test_conv_parity(name, record_property):
    c = CASES[name]
    ratios = run_case(c)
    if ratios:
        record_property("variant", c["target"]["variant"])
        record_property("mode", c["mode"])
        for k, v in ratios.items():
            record_property("ratio_" + k, v)

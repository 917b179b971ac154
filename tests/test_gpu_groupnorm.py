"""vaw_groupnorm_fwd / _apply / _bwd against the float64 reference of tests/gn_parity.py on every launch, group size and edge the case
table names.  Each case sets its switch, asks vaw_gn_plan for the four passes it is about to run and refuses to run on any other
launch, calls the three entry points through the C ABI, compares every element of mean, rstd, y, dx, dgamma, dbeta and the FiLM
gradients against its bound (or exactly, in the exact regime), and runs twice for bitwise-equal results; vaw_groupnorm_apply on the
forward's statistics must write the forward's bytes.  The inputs sit between NaN guards (the FiLM rows between NaN columns), so a read
outside them poisons an output; the outputs sit between canaries, the FiLM gradients inside canary columns; the workspace starts as
NaN before every call; dgamma and dbeta start as NaN at grad_beta 0.  On the quad kernels the bf16 activations sit 8 bytes off a
16-byte boundary: the alignment those kernels ask for and no more."""
import pytest
import torch

import gn_parity as gp
from gn_parity import CASES

pytestmark = pytest.mark.gpu

from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import lib, stream_ptr

DEV = "cuda"
CANARY = 768.0            # exact in bf16
NAN = float("nan")
TDT = gp.TORCH_DT


def _guarded(values, dt, guard, fill):
    """values (float64, any shape) in the middle of a flat buffer with `guard` elements of `fill` on both sides -> (flat, address)"""
    n = values.numel()
    flat = torch.full((n + 2 * guard,), fill, dtype=TDT[dt], device=DEV)
    flat[guard:guard + n] = values.reshape(-1).to(TDT[dt])
    return flat, flat.data_ptr() + guard * flat.element_size()


class _Run:
    """one forward, apply and backward of a case on fresh output buffers"""

    def __init__(self, c, t, ws):
        B, HW, C, G, dt = c["B"], c["HW"], c["C"], c["G"], c["dt"]
        self.c, self.ws, self.keep, self.addr, self.outs = c, ws, [], {}, {}
        self.ag = ag = 64 if c["target"]["variant"] == "flat" else 68          # activations: 136 bytes of bf16 guard on the quad kernels
        self.lay = lay = gp.film_layout(c)

        def inp(name, values, dt_, guard):
            flat, a = _guarded(values, dt_, guard, NAN)
            self.keep.append(flat)
            self.addr[name] = a

        inp("x", t["x"], dt, ag)
        inp("dout", t["dout"], dt, ag)
        if c["add"]:
            inp("dx_add", t["dx_add"], dt, ag)
        inp("gamma", t["gamma"], "f32", 64)
        inp("beta", t["beta"], "f32", 64)
        if c["film"]:
            emb = torch.full_like(t["emb"], NAN)
            for o in lay[1:3]:
                emb[:, o:o + C] = t["emb"][:, o:o + C]
            inp("emb", emb, "f32", 64)

        def out(name, shape, dt_, guard, init=None):
            vals = init if init is not None else torch.full(shape, CANARY, dtype=torch.float64)
            flat, a = _guarded(vals, dt_, guard, CANARY)
            self.addr[name] = a
            self.outs[name] = (flat, flat.clone(), guard, tuple(shape))

        for k in ("y", "ya", "dx"):
            out(k, (B, HW, C), dt, ag)
        out("mean", (B, G), "f32", 64)
        out("rstd", (B, G), "f32", 64)
        out("dgamma", (C,), "f32", 64, t["dgamma_old"])
        out("dbeta", (C,), "f32", 64, t["dbeta_old"])
        out("demb", (B, lay[3]), "f32", 64)

    def launch(self):
        c, a, lay = self.c, self.addr, self.lay
        B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
        dt = L.F32 if c["dt"] == "f32" else L.BF16
        film = bool(c["film"])
        sc, sh = (a["emb"] + 4 * lay[1], a["emb"] + 4 * lay[2]) if film else (None, None)
        dsc, dsh = (a["demb"] + 4 * lay[4], a["demb"] + 4 * lay[5]) if film else (None, None)
        wsp = self.ws.data_ptr()
        self.ws.fill_(NAN)
        assert lib().vaw_groupnorm_fwd(dt, a["x"], a["gamma"], a["beta"], sc, sh, lay[0], int(c["silu"]), a["y"], a["mean"], a["rstd"], B, HW, C, G,
                                       c["eps"], wsp, stream_ptr()) == 0, lib().vaw_last_error_string()
        self.ws.fill_(NAN)
        assert lib().vaw_groupnorm_apply(dt, a["x"], a["mean"], a["rstd"], a["gamma"], a["beta"], sc, sh, lay[0], int(c["silu"]), a["ya"], B, HW, C,
                                         G, stream_ptr()) == 0, lib().vaw_last_error_string()
        self.ws.fill_(NAN)
        assert lib().vaw_groupnorm_bwd(dt, a["dout"], a["x"], a["mean"], a["rstd"], a["gamma"], a["beta"], sc, sh, lay[0], int(c["silu"]),
                                       a.get("dx_add"), a["dx"], a["dgamma"], a["dbeta"], c["grad_beta"], dsc, dsh, lay[3], B, HW, C, G, wsp,
                                       stream_ptr()) == 0, lib().vaw_last_error_string()
        torch.cuda.synchronize()

    def results(self):
        """name -> float64 output; the canaries around every output and around the FiLM gradient columns are checked on the way"""
        c, C, lay, got = self.c, self.c["C"], self.lay, {}
        for k, (flat, init, guard, shape) in self.outs.items():
            n = flat.numel() - 2 * guard
            same = lambda u, v: torch.equal(u.view(torch.uint8), v.view(torch.uint8))
            assert same(flat[:guard], init[:guard]) and same(flat[guard + n:], init[guard + n:]), (c["name"], k, "canaries next to the output were written")
            got[k] = flat[guard:guard + n].view(shape).double()
        demb = got.pop("demb")
        if c["film"]:
            got["dscale"], got["dshift"] = demb[:, lay[4]:lay[4] + C], demb[:, lay[5]:lay[5] + C]
            demb = demb.clone()
            demb[:, lay[4]:lay[4] + C] = CANARY
            demb[:, lay[5]:lay[5] + C] = CANARY
        assert bool((demb == CANARY).all()), (c["name"], "the FiLM gradient rows were written outside dscale / dshift")
        del got["ya"]
        assert torch.equal(self.outs["ya"][0].view(torch.uint8), self.outs["y"][0].view(torch.uint8)), \
            (c["name"], "vaw_groupnorm_apply on the forward's statistics gave other bytes than the forward")
        return got

    def raw(self):
        return [o[0] for o in self.outs.values()]


def run_case(c):
    """-> name -> worst err / bound of each output of the case (asserted <= 1)"""
    t = gp.make_inputs(c)
    dt = L.F32 if c["dt"] == "f32" else L.BF16
    ws = torch.empty(lib().vaw_groupnorm_workspace_floats(c["B"], c["HW"], c["C"]), device=DEV)       # sized before the switch is set
    lib().vaw_debug_gn_flat(c["switch"])
    try:
        for p in (L.GN_FWD_SUMS, L.GN_APPLY, L.GN_BWD_SUMS, L.GN_BWD_APPLY):
            plan = ops.gn_plan(p, dt, c["B"], c["HW"], c["C"], c["G"])
            got_t = gp.describe_plan(c, plan, L)
            assert got_t == c["target"], (c["name"], p, got_t, c["target"])
            assert plan.workspace_floats <= ws.numel(), (c["name"], p)
        a, b = _Run(c, t, ws), _Run(c, t, ws)
        a.launch()
        b.launch()
    finally:
        lib().vaw_debug_gn_flat(-1)
    got = a.results()
    b.results()
    for u, v in zip(a.raw(), b.raw()):            # fixed-order reductions: a repeat is bitwise equal
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (c["name"], "a second run gave other bits")
    td = {k: v.to(DEV) for k, v in t.items()}
    ref, bound = gp.evaluate(c, td)
    ratios = gp.ratios(c, ref, bound, got)
    print("GN", c["name"], c["target"]["variant"], c["dt"], c["regime"], {k: round(v, 4) for k, v in ratios.items()}, flush=True)
    assert max(ratios.values()) <= 1.0, (c["name"], ratios)
    return ratios


@pytest.mark.parametrize("name", list(CASES))
def test_groupnorm_parity(name, record_property):
    c = CASES[name]
    ratios = run_case(c)
    record_property("mapping", c["target"]["variant"])
    record_property("regime", c["regime"])
    for k, v in ratios.items():
        record_property("ratio_" + k, v)

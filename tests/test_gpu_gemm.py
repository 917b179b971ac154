"""vaw_gemm against the float64 reference of tests/gemm_parity.py on every kernel, epilogue kind and edge the case table names: each
case sets its debug tile / generic switch, asks vaw_gemm_plan (the process's own knobs) for the call it is about to make and
refuses to run on any other kernel, launches through ops.gemm with raw pointers (leading dimensions, 2-byte offsets and canaries
are the test's), compares every output element by element against the bound, and runs twice for bitwise-equal results.  The
knobs the library reads from the environment once per process run in fresh children, one after another.  vaw_wgrad_grouped with
per-problem alpha and padded leading dimensions is held to the same accumulation bound.

Run as a script (--child SETTING) this file is such a child: it runs the setting's subset and prints one JSON line."""
import json
import os
import subprocess
import sys

if __name__ == "__main__":
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

import pytest
import torch

import gemm_parity as gp
from gemm_parity import CASES

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF16

DEV = "cuda"
IN_CANARY, OUT_CANARY = 8192.0, 768.0        # exact in bf16; padding of the inputs / of the outputs
GUARD = 64                                   # elements behind every buffer
TDT = gp.TORCH_DT


def _buf(values, ld, dt, off=0, canary=IN_CANARY):
    """values [R][C] (float64) stored with row stride ld from element `off` of a canary-filled buffer -> (flat, address)"""
    R, Cc = values.shape
    flat = torch.full((off + R * ld + GUARD,), canary, dtype=TDT[dt], device=DEV)
    flat[off:off + R * ld].view(R, ld)[:, :Cc] = values.to(TDT[dt])
    return flat, flat.data_ptr() + off * flat.element_size()


def _logical(flat, R, Cc, ld, off):
    return flat[off:off + R * ld].view(R, ld)[:, :Cc]


def _untouched_outside(flat, init, R, Cc, ld, off):
    """everything but the logical [R][Cc] region still holds what it held before the launch"""
    a, b = flat.clone(), init.clone()
    _logical(a, R, Cc, ld, off).zero_()
    _logical(b, R, Cc, ld, off).zero_()
    return torch.equal(a, b)


class _Run:
    """one launch of a case on fresh output buffers"""

    def __init__(self, c, t, part_rows=None):
        g = gp.geometry(c)
        M, N, dt, odt = c["M"], c["N"], c["dt"], gp.out_dt(c)
        off = lambda k: 1 if k in c["off"] else 0
        self.c, self.g, self.keep, self.addr, self.outs = c, g, [], {}, {}

        def inp(name, values, ld, d, o=0):
            flat, a = _buf(values, ld, d, o)
            self.keep.append(flat)
            self.addr[name] = a

        inp("A", t["A"], g["lda"], dt, off("A"))
        inp("B", t["B"], g["ldb"], dt)
        if c["bias"]:
            inp("bias", t["bias"][None], N, "f32")
        if c["act"] == 2:
            inp("aux_in", t["aux_in"], g["ldc"], dt)
        if c["gate"]:
            inp("gate", t["gate"], g["gate_ld"], "f32")
        if c["resid"]:
            inp("resid", t["resid"], g["ldc"], gp.resid_dt(c))
        if c["rowadd"]:
            inp("rowadd", t["rowadd"], N, "f32")

        def out(name, key, R, Cc, ld, d, o=0, init=None):
            vals = init if init is not None else torch.full((R, Cc), OUT_CANARY, dtype=torch.float64)
            flat, a = _buf(vals, ld, d, o, canary=OUT_CANARY)
            self.addr[name] = a
            self.outs[key] = (flat, flat.clone(), R, Cc, ld, o)

        out("C", "C", M, N, g["ldc"], odt, off("C"), t.get("C_old"))
        if c["aux_out"]:
            out("aux_out", "aux_out", M, N, g["ldc"], dt, off("aux_out"))
        if c["colsum"] == "out":
            out("colsum_out", "colsum", 1, N, N, "f32", 0, t["colsum_old"][None])
        if c["rowsum"]:
            out("rowsum_a_out", "rowsum", 1, M, M, "f32", 0, t["rowsum_old"][None])
        self.part = None
        if c["colsum"] == "partial":
            cap = -(-M // 64) if part_rows is None else part_rows
            self.part_big = torch.full((cap + 8, N), OUT_CANARY, device=DEV)
            self.part = ops.ColsumPartial(1, N, torch.device(DEV))
            self.part.buf = self.part_big[:cap]

    def plan(self):
        ws = ops.scratch_f32(torch.device(DEV, torch.cuda.current_device()), 0).numel() if gp.workspace_floats(self.c) else 0
        return gp.plan_of(self.c, L, ops, knobs=None, addr=self.addr, workspace=ws), ws

    def launch(self):
        args, kw = gp.plan_call(self.c, self.addr)
        ops.gemm(*args, colsum_partial=self.part, **kw)
        torch.cuda.synchronize()

    def results(self):
        """name -> float64 logical output; the canaries around every output are checked on the way"""
        got = {}
        for key, (flat, init, R, Cc, ld, o) in self.outs.items():
            assert _untouched_outside(flat, init, R, Cc, ld, o), (self.c["name"], key, "padding or guard elements were written")
            v = _logical(flat, R, Cc, ld, o).double()
            got[key] = v[0] if key in ("colsum", "rowsum") else v
        if self.part is not None:
            R = self.part.rows.value
            assert bool((self.part_big[R:] == OUT_CANARY).all()), (self.c["name"], R, "rows behind the partial buffer were written")
            got["colsum"] = self.part_big[:R].double().sum(0)
        return got

    def raw(self):
        return [o[0] for o in self.outs.values()] + ([self.part_big] if self.part is not None else [])


class _switches:
    def __init__(self, c):
        self.c = c

    def __enter__(self):
        L.lib().vaw_debug_gemm_tile(self.c["tile"])
        L.lib().vaw_debug_force_generic_gemm(self.c["generic"])

    def __exit__(self, *a):
        L.lib().vaw_debug_gemm_tile(-1)
        L.lib().vaw_debug_force_generic_gemm(0)


def _same_target(c, p):
    got = dict(zip(gp.TARGET_FIELDS, gp.describe_plan(L, p)))
    assert got == c["target"], (c["name"], got, c["target"])


def run_case(c, expect=_same_target):
    """-> name -> worst err / bound of each output of the case (asserted <= 1)"""
    t = gp.make_inputs(c)
    td = {k: v.to(DEV) for k, v in t.items()}
    prod = gp.products(c, td)
    with _switches(c):
        a, b = _Run(c, t), _Run(c, t)
        p, ws = a.plan()
        assert p.status == 0
        expect(c, p)
        assert p.workspace_floats_used <= ws, (c["name"], p.workspace_floats_used, ws)
        a.launch()
        b.launch()
        if a.part is not None:
            assert a.part.rows.value == p.colsum_rows, (c["name"], a.part.rows.value, p.colsum_rows)
        else:
            assert (p.colsum_rows > 0) == bool(c["colsum"]), (c["name"], p.colsum_rows)
        got = a.results()
        b.results()
        for x, y in zip(a.raw(), b.raw()):       # fixed-order reductions: a repeat is bitwise equal
            assert torch.equal(x, y), (c["name"], "a second launch gave other bits")
        if a.part is not None and p.colsum_rows > 1:      # a buffer one row short: refused before anything runs, C_old untouched
            r = _Run(c, t, part_rows=p.colsum_rows - 1)
            with pytest.raises(vaw_amd.VawError, match="colsum_partial_out holds"):
                r.launch()
            torch.cuda.synchronize()
            assert torch.equal(r.outs["C"][0], r.outs["C"][1]) and bool((r.part_big == OUT_CANARY).all())
    ratios = gp.ratios(c, td, prod, got)
    print(c["name"], c["target"]["variant"], {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (c["name"], ratios)
    return ratios


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_parity(name, record_property):
    ratios = run_case(CASES[name])
    record_property("variant", CASES[name]["target"]["variant"])
    record_property("worst_ratio", max(ratios.values()))
    for k, v in ratios.items():
        record_property("ratio_" + k, v)


# ------------------------------------------------------------------------------------------------------------------------------
# knobs read from the environment once per process: fresh children
# ------------------------------------------------------------------------------------------------------------------------------
def _expect_bk32(c, p):
    want = dict(c["target"], variant="t128_bk32")
    got = dict(zip(gp.TARGET_FIELDS, gp.describe_plan(L, p)))
    assert got == want, (c["name"], got, want)


def _expect_no_xcd(c, p):
    assert p.xcd_parts == 0 and p.split > 1 and L.GV_NAMES[p.variant] == c["target"]["variant"], (c["name"], p.xcd_parts, p.split)


def _expect_8_loaders(c, p):
    assert p.block == 1024 and L.GV_NAMES[p.variant] == "warp_spec" and p.ntw == 3, (c["name"], p.block, p.ntw)


def _expect_3_stages(c, p):
    want = dict(c["target"], sm=c["target"]["sm"][:2] + (3,))
    got = dict(zip(gp.TARGET_FIELDS, gp.describe_plan(L, p)))
    assert got == want, (c["name"], got, want)


_T = lambda pred: [n for n, c in CASES.items() if pred(c, c["target"])]
ENV_RUNS = {
    # setting -> (cases, what the plan must say under it)
    "VAW_GEMM_EPI=0": (_T(lambda c, t: t["variant"].startswith("t128")), _same_target),      # LDS-staged epilogue on every kind
    "VAW_GEMM_BK=32": (_T(lambda c, t: t["variant"] == "t128_bk64" and c["tile"] == 0), _expect_bk32),
    "VAW_GEMM_XCDSPLIT=0": (_T(lambda c, t: t["variant"] == "t128_bk64" and t["split"]), _expect_no_xcd),
    "VAW_WS_LOADERS=8": (_T(lambda c, t: t["variant"] == "warp_spec" and t["ntw"] == 3), _expect_8_loaders),
    "VAW_SM_STAGES=3": (_T(lambda c, t: t["variant"] == "small_m"), _expect_3_stages),
}
# the same settings as fields of vaw_gemm_knobs: test_gemm_parity_cpu.py holds the expectations to the plan without a GPU
ENV_KNOBS = {"VAW_GEMM_EPI=0": dict(epi=0), "VAW_GEMM_BK=32": dict(bk=32), "VAW_GEMM_XCDSPLIT=0": dict(xcdsplit=0),
             "VAW_WS_LOADERS=8": dict(ws_loaders=8), "VAW_SM_STAGES=3": dict(sm_stages=3)}
_child_died = []


@pytest.mark.parametrize("setting", list(ENV_RUNS))
def test_gemm_parity_env_knob(setting, record_property):
    """The setting's cases in a fresh child with the variable in its environment (same functions, the plan checked under the
    knob).  A child that ends on a signal, an abort or a time limit fails the test, and no further child is started."""
    if _child_died:
        pytest.fail(f"not started: the child of {_child_died[0]} died")
    names, _ = ENV_RUNS[setting]
    assert len(names) >= 3, (setting, names)
    k, v = setting.split("=")
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting], env={**os.environ, k: v}, capture_output=True,
                              text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _child_died.append(setting)
        pytest.fail(f"{setting}: child timed out")
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _child_died.append(setting)
    assert proc.returncode == 0, (setting, proc.returncode, proc.stdout[-3000:], proc.stderr[-3000:])
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert sorted(res["worst"]) == sorted(names) and max(res["worst"].values()) <= 1.0, res
    record_property("worst_ratio", max(res["worst"].values()))


def _child(setting):
    names, expect = ENV_RUNS[setting]
    k, v = setting.split("=")
    assert os.environ.get(k) == v
    worst = {n: max(run_case(CASES[n], expect).values()) for n in names}
    print(json.dumps({"setting": setting, "worst": worst}))


# ------------------------------------------------------------------------------------------------------------------------------
# vaw_wgrad_grouped: random data, per-problem alpha, padded leading dimensions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["alpha", "ld_padded"])
def test_wgrad_grouped_float64(case, record_property):
    """dW_p = beta dW_p + alpha_p dy_p^T x_p on random bf16 data: whole tiles, K-split tiles and edge tiles in M and N, held to
    c (K u |alpha| |dy|^T |x| + 8 u (|alpha| |dy|^T |x| + |beta dW_old|)) + u |dW|; padding of dW keeps its canary."""
    g = torch.Generator().manual_seed(7 if case == "alpha" else 8)
    K, beta = 320, 0.5
    shapes = [(200, 264, 0.25), (520, 72, -1.5), (136, 1000, 3.0)] if case == "alpha" else [(200, 264, 0.5), (136, 72, 1.0)]
    pad = (0, 0, 0) if case == "alpha" else (8, 16, 8)
    probs, chk = [], []
    for (M, N, alpha) in shapes:
        dy = gp.rnd(torch.randn(K, M, generator=g, dtype=torch.float64), "bf16")
        x = gp.rnd(torch.randn(K, N, generator=g, dtype=torch.float64), "bf16")
        dw0 = gp.rnd(torch.randn(M, N, generator=g, dtype=torch.float64), "f32")
        fd, ad = _buf(dy, M + pad[0], "bf16")
        fx, ax = _buf(x, N + pad[1], "bf16")
        fw, aw = _buf(dw0, N + pad[2], "f32", canary=OUT_CANARY)
        probs.append((ad, ax, aw, M, N, M + pad[0], N + pad[1], N + pad[2], alpha))
        chk.append((fd, fx, fw, fw.clone(), dy, x, dw0, M, N, alpha))
    grp = ops.WgradGroup(probs, K, torch.device(DEV))
    grp.launch(BF16, beta)
    torch.cuda.synchronize()
    worst = 0.0
    for fd, fx, fw, init, dy, x, dw0, M, N, alpha in chk:
        assert _untouched_outside(fw, init, M, N, N + pad[2], 0), (case, M, N)
        got = _logical(fw, M, N, N + pad[2], 0).double().cpu()
        prod, absprod = dy.t() @ x, dy.t().abs() @ x.abs()
        ref = beta * dw0 + alpha * prod
        mag = abs(alpha) * absprod + (beta * dw0).abs()
        bound = gp.C_BOUND["bf16"] * (K * gp.U32 * abs(alpha) * absprod + gp.EPI_F32_OPS * gp.U32 * mag) + gp.U32 * ref.abs()
        r = float(((got - ref).abs() / bound).max())
        print(case, M, N, alpha, round(r, 4))
        worst = max(worst, r)
    record_property("worst_ratio", worst)
    assert worst <= 1.0, (case, worst)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])

"""vaw_gemm_fp8 against the float64 reference of tests/gemm_parity.py on every kernel instantiation (epilogue kind x operand format x
tile width) and edge the table FP8_CASES names: each case asks vaw_gemm_fp8_plan for the call it is about to make and refuses to run
on any other instantiation, launches twice on fresh buffers through raw pointers (leading dimensions, paddings and canaries are the
test's), compares every output element by element against the bound, and holds the fp8-output kinds bitwise to the bf16 launch
followed by vaw_fp8_quantize_delayed.  vaw_wgrad_grouped with fp8 operands is held to the same accumulation bound."""
import ctypes as C

import pytest
import torch

import gemm_parity as gp
from gemm_parity import FP8_CASES

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF16, BF8, FP8

DEV = "cuda"
IN_CANARY, OUT_CANARY, BYTE_CANARY = 8192.0, 768.0, 0x5A      # exact in bf16; 0x5A is a finite value in both fp8 formats
GUARD = 64                                                    # elements behind every buffer
TDT = dict(gp.TORCH_DT, u8=torch.uint8)
CODE = {"e4m3": FP8, "e5m2": BF8}


def _buf(values, ld, dt, canary):
    """values [R][C] stored with row stride ld in a canary-filled buffer -> flat tensor"""
    R, Cc = values.shape
    flat = torch.full((R * ld + GUARD,), canary, dtype=TDT[dt], device=DEV)
    flat[:R * ld].view(R, ld)[:, :Cc] = values.to(device=DEV, dtype=TDT[dt])
    return flat


def _fp8_buf(values, ld, fmt):
    """fp8 values as bytes; the padding holds the format's largest finite byte pattern"""
    return _buf(gp.fp8_bytes(values.cpu(), fmt), ld, "u8", gp.FMAX_BYTE[fmt])


def _logical(flat, R, Cc, ld):
    return flat[:R * ld].view(R, ld)[:, :Cc]


def _untouched_outside(flat, init, R, Cc, ld):
    a, b = flat.clone(), init.clone()
    _logical(a, R, Cc, ld).zero_()
    _logical(b, R, Cc, ld).zero_()
    return torch.equal(a, b)


class _State:
    """what ops.gemm_fp8 takes as out_fp8: a delayed-scaling state and its format"""

    def __init__(self, scale, fmt, amax=0.0):
        self.state = torch.tensor([float(scale), amax, gp.FMAX[fmt] / 2.0, 123.0], dtype=torch.float32, device=DEV)
        self.init = self.state.clone()
        self.fmt = CODE[fmt]


class _Run:
    """one launch of a case on fresh output buffers; q = False runs the twin of a *_Q case that writes C as bf16"""

    def __init__(self, c, t, q=True, part_rows=None, amax=0.0):
        g = gp.geometry(c)
        M, N, K = c["M"], c["N"], c["K"]
        self.c, self.g, self.keep, self.addr, self.outs = c, g, [], {}, {}
        self.q = c["q_fmt"] if q else None
        self.part_rows = part_rows

        def inp(name, flat):
            self.keep.append(flat)
            self.addr[name] = flat.data_ptr()

        inp("A", _fp8_buf(t["A"], g["lda"], c["a_fmt"]))
        inp("B", _fp8_buf(t["B"], g["ldb"], "e4m3"))
        inp("scale_a", torch.tensor([c["scale_a"]], dtype=torch.float32, device=DEV))
        inp("scale_b", torch.tensor([c["scale_b"]], dtype=torch.float32, device=DEV))
        if c["bias"]:
            inp("bias", _buf(t["bias"][None], N, "f32", IN_CANARY))
        if c["act"] == 2:
            inp("aux_in", _buf(t["aux_in"], g["ldc"], "bf16", IN_CANARY))
        if c["gate"]:
            inp("gate", _buf(t["gate"], g["gate_ld"], "f32", IN_CANARY))
            inp("resid", _buf(t["resid"], g["ldc"], "f32", IN_CANARY))

        def out(name, key, R, Cc, ld, d, canary=OUT_CANARY, init=None):
            vals = init if init is not None else torch.full((R, Cc), canary, dtype=torch.float64)
            flat = _buf(vals, ld, d, canary)
            self.addr[name] = flat.data_ptr()
            self.outs[key] = (flat, flat.clone(), R, Cc, ld)

        if self.q:
            out("C", "Cq", M, N, g["ldc"], "u8", BYTE_CANARY)         # bytes: ldc is the row stride in bytes
        else:
            out("C", "C", M, N, g["ldc"], gp.out_dt(c))
        if c["aux_out"]:
            out("aux_out", "aux_out", M, N, g["ldc"], "bf16")
        if c["colsum"] == "out":
            out("colsum_out", "colsum", 1, N, N, "f32", init=t["colsum_old"][None])
        self.part = None
        if c["colsum"] == "partial":
            cap = -(-M // 128) if part_rows is None else part_rows
            self.part_big = torch.full((cap + 8, N), OUT_CANARY, device=DEV)
            self.part = ops.ColsumPartial(1, N, torch.device(DEV))
            self.part.buf = self.part_big[:cap]
        self.st = _State(float(t["q_scale"]), self.q, amax) if self.q else None

    def plan(self, **kw):
        ws = ops.scratch_f32(torch.device(DEV, torch.cuda.current_device()), 0).numel() if self.c["colsum"] == "out" else 0
        c = self.c if self.q else dict(self.c, q_fmt=None)
        return gp.fp8_plan_of(c, ops, cus=0, addr=self.addr, workspace=ws, q_state=self.st.state.data_ptr() if self.q else 0,
                              part_rows=self.part_rows, **kw), ws

    def launch(self):
        args, kw = gp.fp8_plan_call(self.c, self.addr)
        ops.gemm_fp8(*args, colsum_partial=self.part, out_fp8=self.st, **kw)
        torch.cuda.synchronize()

    def results(self):
        """name -> float64 logical output (Cq: the decoded bytes times the scale); canaries around every output are checked on the way"""
        got = {}
        for key, (flat, init, R, Cc, ld) in self.outs.items():
            assert _untouched_outside(flat, init, R, Cc, ld), (self.c["name"], key, "padding or guard elements were written")
            v = _logical(flat, R, Cc, ld)
            if key == "Cq":
                got[key] = gp.fp8_decode(v.cpu().contiguous(), self.q).to(DEV) * float(self.st.init[0])
            else:
                got[key] = v.double()[0] if key == "colsum" else v.double()
        if self.part is not None:
            R = self.part.rows.value
            assert bool((self.part_big[R:] == OUT_CANARY).all()), (self.c["name"], R, "rows behind the partial buffer were written")
            got["colsum"] = self.part_big[:R].double().sum(0)
        if self.st is not None:
            s, s0 = self.st.state, self.st.init
            assert torch.equal(s[[0, 2, 3]].view(torch.int32), s0[[0, 2, 3]].view(torch.int32)), (self.c["name"], "state[0], [2] or [3] changed")
            got["amax"] = s[1].double()
        return got

    def raw(self):
        return [o[0] for o in self.outs.values()] + ([self.part_big] if self.part is not None else []) + \
               ([self.st.state] if self.st is not None else [])


class _grid_of_16:
    """the persistent grids of the process on 16 CUs, for the cases that run more than one item per workgroup"""

    def __init__(self, c):
        self.on = c["cus"] == 16

    def __enter__(self):
        if self.on:
            L.lib().vaw_p8_set_reserved_cus(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count - 16)

    def __exit__(self, *a):
        L.lib().vaw_p8_set_reserved_cus(0)


def _same_target(c, p):
    got = dict(zip(gp.FP8_TARGET_FIELDS, gp.describe_fp8_plan(L, p)))
    assert p.status == 0 and got == c["target"], (c["name"], got, c["target"])
    if c["target"]["rounds"]:
        assert p.grid == 16 and p.tiles_m * p.tiles_n > p.grid, (c["name"], p.grid, p.tiles_m, p.tiles_n)


def run_case(c):
    """-> name -> worst err / bound of each output of the case (asserted <= 1)"""
    t = gp.make_fp8_inputs(c)
    td = {k: v.to(DEV) for k, v in t.items()}
    prod = gp.products(c, td)
    share = gp.prepare_q(c, td, prod)
    if c["q_fmt"]:
        assert 0.001 <= share <= 0.05, (c["name"], share)
    try:
        with _grid_of_16(c):
            a, b = _Run(c, td), _Run(c, td)
            p, ws = a.plan()
            _same_target(c, p)
            assert p.workspace_floats_used <= ws and bool(p.c_fp8) == bool(c["q_fmt"]), (c["name"], p.workspace_floats_used, ws)
            a.launch()
            b.launch()
            if a.part is not None:
                assert a.part.rows.value == p.colsum_rows, (c["name"], a.part.rows.value, p.colsum_rows)
            got = a.results()
            b.results()
            for x, y in zip(a.raw(), b.raw()):       # fixed-order reductions, an order-independent max: a repeat is bitwise equal
                assert torch.equal(x, y), (c["name"], "a second launch gave other bits")
            if c["q_fmt"]:
                got["C"] = _check_against_twin(c, td, a)
            if a.part is not None and p.colsum_rows > 1:      # a buffer one row short: refused before anything runs, nothing written
                r = _Run(c, td, part_rows=p.colsum_rows - 1)
                assert r.plan(check_status=False)[0].status == -1
                with pytest.raises(vaw_amd.VawError, match="colsum_partial_out holds"):
                    r.launch()
                torch.cuda.synchronize()
                assert all(torch.equal(o[0], o[1]) for o in r.outs.values()) and bool((r.part_big == OUT_CANARY).all())
    finally:
        L.lib().vaw_p8_set_reserved_cus(0)
    ratios = gp.ratios(c, td, prod, got)
    print(c["name"], tuple(c["target"].values()), {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (c["name"], ratios)
    return ratios


def _check_against_twin(c, td, a):
    """The *_Q launch == its twin with a bf16 C followed by vaw_fp8_quantize_delayed on that C with a copy of the state: bytes,
    state[1], aux_out and the column sums bitwise; a running max preset above the tensor's stays.  -> the twin's C (float64)"""
    M, N, ldc = c["M"], c["N"], a.g["ldc"]
    tw = _Run(c, td, q=False)
    _same_target(dict(c, target=dict(c["target"], epi_kind=c["target"]["epi_kind"][:-2])), tw.plan()[0])
    tw.launch()
    got = tw.results()
    for key in ("aux_out", "colsum"):
        if key in a.outs:
            assert torch.equal(a.outs[key][0], tw.outs[key][0]), (c["name"], key, "differs from the bf16 launch's")
    if a.part is not None:
        assert a.part.rows.value == tw.part.rows.value and torch.equal(a.part_big, tw.part_big), (c["name"], "partial column sums")
    st = _State(float(td["q_scale"]), c["q_fmt"])
    q = torch.full((M * ldc + GUARD,), BYTE_CANARY, dtype=torch.uint8, device=DEV)
    ops.check(L.lib().vaw_fp8_quantize_delayed(BF16, st.fmt, tw.outs["C"][0].data_ptr(), M, N, ldc, q.data_ptr(), ldc, None, 0,
                                               st.state.data_ptr(), L.stream_ptr()), "vaw_fp8_quantize_delayed")
    torch.cuda.synchronize()
    assert torch.equal(q, a.outs["Cq"][0]), (c["name"], "bytes differ from vaw_fp8_quantize_delayed of the bf16 C")
    assert torch.equal(st.state.view(torch.int32), a.st.state.view(torch.int32)), (c["name"], st.state, a.st.state)
    assert float(st.state[1]) == float(got["C"].abs().max())
    preset = 2.0 * float(st.state[1])
    hi = _Run(c, td, amax=preset)
    hi.launch()
    hi.results()
    assert float(hi.st.state[1]) == preset and torch.equal(hi.outs["Cq"][0], a.outs["Cq"][0]), (c["name"], hi.st.state)
    return got["C"]


@pytest.mark.parametrize("name", list(FP8_CASES))
def test_gemm_fp8_parity(name, record_property):
    ratios = run_case(FP8_CASES[name])
    record_property("kind", "/".join(map(str, FP8_CASES[name]["target"].values())))
    record_property("worst_ratio", max(ratios.values()))
    for k, v in ratios.items():
        record_property("ratio_" + k, v)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: the call and the plan alike, and nothing is written
# ------------------------------------------------------------------------------------------------------------------------------
def test_gemm_fp8_refusals_write_nothing():
    from test_gemm_fp8_parity_cpu import REFUSALS
    big = lambda dt, canary: torch.full((1 << 18,), canary, dtype=dt, device=DEV)
    A, B, aux = big(torch.uint8, 0x7E), big(torch.uint8, 0x7E), big(torch.bfloat16, IN_CANARY)
    f32 = big(torch.float32, IN_CANARY)
    sa, sb = torch.tensor([0.3], device=DEV), torch.tensor([1.7], device=DEV)
    ws = ops.scratch_f32(torch.device(DEV, torch.cuda.current_device()), 0)
    for name, (M, N, K, lda, ldb, ldc, kw, status, text) in REFUSALS.items():
        Cb, aux_o, cs = big(torch.float32, OUT_CANARY), big(torch.bfloat16, OUT_CANARY), big(torch.float32, OUT_CANARY)
        st = _State(0.01, "e4m3")
        kw = dict(kw)
        ptrs = dict(bias=f32, aux_in=aux, aux_out=aux_o, gate=f32, resid=f32, colsum_out=cs)
        real = {k: (ptrs[k].data_ptr() if k in ptrs else v) for k, v in kw.items() if k not in ("out_fp8_state", "colsum_partial_rows", "workspace_floats")}
        args = (M, N, K, A.data_ptr(), lda, sa.data_ptr(), B.data_ptr(), ldb, sb.data_ptr(), Cb.data_ptr(), ldc)
        part = None
        if "colsum_partial_rows" in kw:
            part = ops.ColsumPartial(1, N, torch.device(DEV))
            part.buf = cs[:kw["colsum_partial_rows"] * N].view(-1, N)
        has_ws = "colsum_out" in kw and name != "colsum_no_workspace"
        p = ops.gemm_fp8_plan(*args, check_status=False, out_fp8_state=st.state.data_ptr() if "out_fp8_state" in kw else 0,
                              colsum_partial_rows=kw.get("colsum_partial_rows"), workspace=ws.data_ptr(), workspace_floats=ws.numel() if has_ws else 0,
                              **real)
        assert p.status == status and L.lib().vaw_last_error_string().decode() == text, (name, p.status)
        if name == "colsum_no_workspace":
            continue              # ops.gemm_fp8 always hands a workspace to a call with colsum_out: the plan alone can be asked
        with pytest.raises(vaw_amd.VawError) as ei:
            ops.gemm_fp8(*args, colsum_partial=part, out_fp8=st if "out_fp8_state" in kw else None, **real)
        assert text in str(ei.value), (name, str(ei.value))
        torch.cuda.synchronize()
        for x in (Cb, aux_o, cs):
            assert bool((x == OUT_CANARY).all()), (name, "a refused call wrote")
        assert torch.equal(st.state, st.init), name


# ------------------------------------------------------------------------------------------------------------------------------
# vaw_wgrad_grouped with fp8 operands: random data, per-problem alpha and scales, padded leading dimensions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("case", ["alpha", "ld_padded"])
def test_wgrad_grouped_fp8_float64(case, dy_fmt, record_property):
    """dW_p = beta dW_p + alpha_p s_dy s_x dy_p^T x_p on random fp8 data (dy^T [M][K] of dy_fmt, x^T [N][K] e4m3, both k-major): whole
    tiles, K-split tiles (case alpha: K = 1024) and edge tiles in M and N, held to
    c (K u |a| |dy|^T |x| + 8 u (|a| |dy|^T |x| + |beta dW_old|)) + u |dW| with a = alpha s_dy s_x; padding of dW keeps its canary."""
    g = torch.Generator().manual_seed(17 if case == "alpha" else 18)
    beta = 0.5
    K = 1024 if case == "alpha" else 384
    shapes = [(200, 264, 0.25), (520, 72, -1.5), (136, 1000, 3.0)] if case == "alpha" else [(200, 264, 0.5), (136, 72, 1.0)]
    pad = (0, 0, 0) if case == "alpha" else (16, 16, 8)
    probs, chk, keep = [], [], []
    for i, (M, N, alpha) in enumerate(shapes):
        dy = gp.rnd(torch.randn(M, K, generator=g, dtype=torch.float64), dy_fmt)
        x = gp.rnd(torch.randn(N, K, generator=g, dtype=torch.float64), "e4m3")
        dw0 = gp.rnd(torch.randn(M, N, generator=g, dtype=torch.float64), "f32")
        s_dy, s_x = 0.3 + 0.07 * i, 1.7 / K ** 0.5 - 0.003 * i
        fd, fx = _fp8_buf(dy, K + pad[0], dy_fmt), _fp8_buf(x, K + pad[1], "e4m3")
        fw = _buf(dw0, N + pad[2], "f32", OUT_CANARY)
        sd, sx = torch.tensor([s_dy], dtype=torch.float32, device=DEV), torch.tensor([s_x], dtype=torch.float32, device=DEV)
        keep += [fd, fx, sd, sx]
        probs.append((fd.data_ptr(), fx.data_ptr(), fw.data_ptr(), M, N, K + pad[0], K + pad[1], N + pad[2], alpha, 0, sd.data_ptr(), sx.data_ptr()))
        chk.append((fw, fw.clone(), dy.to(DEV), x.to(DEV), dw0.to(DEV), M, N, alpha * float(sd.double()) * float(sx.double())))
    grp = ops.WgradGroup(probs, K, torch.device(DEV))
    grp.launch(CODE[dy_fmt], beta)
    torch.cuda.synchronize()
    worst = 0.0
    for fw, init, dy, x, dw0, M, N, a in chk:
        assert _untouched_outside(fw, init, M, N, N + pad[2]), (case, M, N)
        got = _logical(fw, M, N, N + pad[2]).double()
        prod, absprod = dy @ x.t(), dy.abs() @ x.abs().t()
        ref = beta * dw0 + a * prod
        mag = abs(a) * absprod + (beta * dw0).abs()
        bound = gp.C_BOUND["fp8"] * (K * gp.U32 * abs(a) * absprod + gp.EPI_F32_OPS * gp.U32 * mag) + gp.U32 * ref.abs()
        r = float(((got - ref).abs() / bound).max())
        print(case, dy_fmt, M, N, round(r, 4))
        worst = max(worst, r)
    record_property("worst_ratio", worst)
    assert worst <= 1.0, (case, dy_fmt, worst)

"""The DiT block's row kernels (csrc/layernorm.hip) against float64 references, through their C entry points, over the launch space
they dispatch on: every NV bucket of D (with a partial last slab in each), one workgroup per sample, samples cut into chunks with a
short last one, fewer rows than waves, T = 1, an odd number of rows per wave, both modulation strides DiT uses, dres_in absent /
separate / aliased to dx, with and without the bias-gradient partials and the workspace.  Every case asserts, through vaw_row_plan,
the kernel variant, NV and row split it means to cover, so a later change of the shape rules cannot silently empty it.

Tolerances follow the precision of each output: f32 outputs rtol 1e-5 with an absolute floor of 1e-5 x rms (per-row values) or
1e-5 x sqrt(T) x rms of the summands (per-sample sums); bf16 outputs within one bf16 ulp of the float64 value (plus the same f32
floor: a value produced by cancellation carries the f32 arithmetic's absolute error before it is rounded); fp8 outputs are the
bytes vaw_fp8_quantize_delayed makes of the bf16 values."""
import math

import pytest
import torch
import torch.nn.functional as F

import model_grad_cases as grad_cases
from conftest import assert_fingerprints, fingerprint, perturb_

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF8, BF16, F32, FP8, lib, ptr, stream_ptr

DEV = "cuda"
EPS = 1e-6
WIDTHS = [4, 60, 256, 260, 516, 772, 1028, 1152, 1204, 1208, 1216, 1280, 1284, 1540, 2048]
# name -> (B, T, workspace): the row splits of the launch plan (asserted in _check_split)
REGIMES = {"one_wg": (256, 9, True),           # one workgroup per sample (B >= 256; T < 16 keeps the 512-workgroup target at nc = 1)
           "split_short": (2, 100, True),      # nc = 12 chunks of 9 rows, the last one holds 1 row
           "few_waves": (3, 5, True),          # T < 8: 5 waves
           "t1": (4, 1, True),                 # one row per sample
           "odd_rows": (2, 24, False)}         # no workspace: nc = 1, 24 rows over 8 waves = 3 rows each (odd: the unrolled-by-two loop's tail)
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
FMT = {"e4m3": FP8, "e5m2": BF8}


def _nv(D):
    nv = -(-D // 256)
    return nv if nv <= 6 else 8


def _case(D, regime):
    """(mod_ld, block offset of the operands in a modulation row, dres mode, bias-gradient partials wanted) for this case: cycled
    over the grid so that every width and every regime meets each choice."""
    ci = WIDTHS.index(D) * len(REGIMES) + list(REGIMES).index(regime)
    depth = 3
    mod_ld, base = ((6 * D, 0), ((6 * depth + 2) * D, 6 * D))[ci % 2]        # dit.py: block l's six chunks at 6*l*D of (6*depth+2)*D
    return mod_ld, base, ("none", "separate", "alias")[ci % 3], (ci // 2) % 2 == 0


def _data(B, T, D, mod_ld, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * T
    return dict(x=torch.randn(M, D, generator=g) * 2 + 0.5, mod=torch.randn(B, mod_ld, generator=g) * 0.5,
                dout=torch.randn(M, D, generator=g), dres=torch.randn(M, D, generator=g), y=torch.randn(M, D, generator=g))


def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def _close_f32(got, ref, floor, what):
    """|got - ref| <= 1e-5 |ref| + floor (f32 arithmetic / accumulation)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    bad = err > 1e-5 * ref.abs() + floor
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {err.numel()} beyond rtol 1e-5, atol {floor:.3g}: max err "
                                 f"{float(err.max()):.3g} at {int(err.argmax())} (ref {float(ref.flatten()[int(err.argmax())]):.6g})")


def _close_bf16(got, ref, floor, what):
    """within one bf16 ulp of the float64 value (+ the f32 floor, see the module docstring)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    ulp = torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120))) - 7)
    err = (got - ref).abs()
    bad = err > ulp + floor
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {err.numel()} beyond one bf16 ulp: max err / ulp "
                                 f"{float((err / ulp).max()):.3g}")


def _close_out(dt, got, ref, floor, what):
    (_close_f32 if dt == F32 else _close_bf16)(got, ref, floor, what)


def _plan(kind, dt, B, T, D, ws):
    return ops.row_plan(kind, dt, B, T, D, workspace_floats=ws.numel() if ws is not None else 0)


def _check_split(p, regime, B, T, D, what):
    """the plan covers what the regime is meant to cover"""
    nw = p.block // 64
    assert p.nv == _nv(D), what
    if regime == "one_wg":
        assert p.nc == 1 and B >= 256, what
    elif regime == "split_short":
        assert p.nc == 12 and p.rows_per_chunk == 9 and T - (p.nc - 1) * p.rows_per_chunk == 1, what
    elif regime == "few_waves":
        assert p.nc == 1 and nw == T < 8, what
    elif regime == "t1":
        assert p.nc == 1 and nw == 1, what
    else:
        assert p.nc == 1 and any(len(range(w, T, nw)) % 2 == 1 for w in range(nw)), what


def _wsargs(ws):
    return (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)


def _twice(fn):
    """run twice: every output bitwise equal (determinism), return the first"""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two runs of the same call differ"
    return a


def _ln_ref(x, shift, scale, dout, B, T, D):
    """float64: modulate(LayerNorm(x)) and autograd's dx, dshift, dscale for the incoming gradient dout"""
    xr, sh, sc = (t.double().clone().requires_grad_(True) for t in (x, shift, scale))
    out = F.layer_norm(xr, (D,), eps=EPS).view(B, T, D) * (1 + sc[:, None]) + sh[:, None]
    (out.reshape(B * T, D) * dout.double()).sum().backward()
    return out.detach().reshape(B * T, D), xr.grad, sh.grad, sc.grad


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_row_kernels_vs_float64(dt, D, regime):
    """vaw_ln_modulate_fwd, vaw_ln_modulate_bwd, vaw_gate_bwd and vaw_ln_modulate_bwd_gate against float64, deterministic, and the
    fused pass bitwise the pair wherever it promises to be (D <= 1280)."""
    B, T, use_ws = REGIMES[regime]
    M = B * T
    mod_ld, base, dres_mode, want_cp = _case(D, regime)
    tdt = TORCH_DT[dt]
    h = _data(B, T, D, mod_ld, seed=D * 7 + T)
    dout_h, y_h = h["dout"].to(tdt), h["y"].to(tdt)                  # the exact operands the kernels see
    x, mod, dout, dres, y = h["x"].to(DEV), h["mod"].to(DEV), dout_h.to(DEV), h["dres"].to(DEV), y_h.to(DEV)
    sh_o, sc_o, g_o, gn_o = base + 3 * D, base + 4 * D, base + 5 * D, base + 2 * D     # shift | scale | gate | gate of the next branch
    shift, scale, gate, gate_n = (h["mod"][:, o:o + D].double() for o in (sh_o, sc_o, g_o, gn_o))
    ws = ops._row_ws(B, T, D) if use_ws else None
    tag = f"dt={dt} D={D} {regime} mod_ld={mod_ld} dres={dres_mode} cp={want_cp}"
    # --- the launches this case means to cover
    p_f = _plan(L.ROW_LN_FWD, dt, B, T, D, ws)
    assert p_f.variant == L.RV_LN_FWD and p_f.nv == _nv(D)
    p_b, p_g, p_u = (_plan(k, dt, B, T, D, ws) for k in (L.ROW_LN_BWD, L.ROW_GATE_BWD, L.ROW_LN_BWD_GATE))
    assert (p_b.variant, p_g.variant) == (L.RV_ROW_BWD, L.RV_ROW_GATE)
    fits = (2 + 4 * (p_u.block // 64)) * D * 4 <= 160 * 1024
    assert p_u.variant == (L.RV_ROW_FUSE8 if dt == BF16 and _nv(D) <= 5 and fits else L.RV_ROW_FUSE), tag
    for p in (p_b, p_g, p_u):
        _check_split(p, regime, B, T, D, tag)
    if D <= 1280:
        assert (p_b.nc, p_b.block) == (p_g.nc, p_g.block) == (p_u.nc, p_u.block), tag

    # --- forward
    def fwd():
        out = torch.empty(M, D, device=DEV, dtype=tdt)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        ops.check(lib().vaw_ln_modulate_fwd(dt, ptr(x), ptr(mod) + 4 * sh_o, ptr(mod) + 4 * sc_o, mod_ld, ptr(out), ptr(mean), ptr(rstd),
                                            B, T, D, EPS, stream_ptr()), "vaw_ln_modulate_fwd")
        torch.cuda.synchronize()
        return out, mean, rstd
    out, mean, rstd = _twice(fwd)
    ref_out, ref_dx, ref_dsh, ref_dsc = _ln_ref(h["x"], shift, scale, dout_h, B, T, D)
    xd = h["x"].double()
    _close_out(dt, out, ref_out, 1e-5 * _rms(ref_out), "out " + tag)
    _close_f32(mean, xd.mean(1), 1e-5 * _rms(xd), "mean " + tag)
    ref_rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + EPS)
    _close_f32(rstd, ref_rstd, 1e-5 * _rms(ref_rstd), "rstd " + tag)

    ref_dx = ref_dx + (h["dres"].double() if dres_mode != "none" else 0.0)
    dxh = dout_h.double().view(B, T, D)
    sum_floor = math.sqrt(T) * 1e-5

    # --- LayerNorm backward
    def ln_bwd():
        dmod = torch.zeros(B, mod_ld, device=DEV)
        dx = dres.clone() if dres_mode == "alias" else torch.empty(M, D, device=DEV)
        dres_in = {"none": None, "separate": ptr(dres), "alias": ptr(dx)}[dres_mode]
        ops.check(lib().vaw_ln_modulate_bwd(dt, ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(mod) + 4 * sc_o, mod_ld, dres_in, ptr(dx),
                                            ptr(dmod) + 4 * sh_o, ptr(dmod) + 4 * sc_o, mod_ld, B, T, D, *_wsargs(ws), stream_ptr()),
                  "vaw_ln_modulate_bwd")
        torch.cuda.synchronize()
        return dx, dmod
    dx, dmod = _twice(ln_bwd)
    _close_f32(dx, ref_dx, 1e-5 * _rms(ref_dx), "dx " + tag)
    xh = (xd - xd.mean(1, keepdim=True)) * ref_rstd[:, None]
    _close_f32(dmod[:, sh_o:sh_o + D], ref_dsh, sum_floor * _rms(dxh), "dshift " + tag)
    _close_f32(dmod[:, sc_o:sc_o + D], ref_dsc, sum_floor * _rms(dxh.reshape(M, D) * xh), "dscale " + tag)
    assert float(dmod[:, :sh_o].abs().max() if sh_o else 0.0) == 0.0 and float(dmod[:, sc_o + D:].abs().max()) == 0.0, tag

    # --- gate backward (of dres, the gradient reaching the gated residual add)
    def gate_bwd():
        dmod_g = torch.zeros(B, mod_ld, device=DEV)
        dy = torch.empty(M, D, device=DEV, dtype=tdt)
        cp = torch.empty(B, D, device=DEV) if want_cp else None
        ops.check(lib().vaw_gate_bwd(dt, ptr(dres), ptr(y), ptr(mod) + 4 * g_o, mod_ld, ptr(dy), ptr(dmod_g) + 4 * g_o, mod_ld,
                                     ptr(cp) if want_cp else None, B, T, D, *_wsargs(ws), stream_ptr()), "vaw_gate_bwd")
        torch.cuda.synchronize()
        return (dy, dmod_g) + ((cp,) if want_cp else ())
    r = _twice(gate_bwd)
    dy, dmod_g = r[0], r[1]
    ref_dy = (h["dres"].double().view(B, T, D) * gate[:, None]).reshape(M, D)
    _close_out(dt, dy, ref_dy, 1e-5 * _rms(ref_dy), "gate dy " + tag)
    terms = h["dres"].double().view(B, T, D) * y_h.double().view(B, T, D)
    _close_f32(dmod_g[:, g_o:g_o + D], terms.sum(1), sum_floor * _rms(terms), "dgate " + tag)
    if want_cp:      # the column sums of dy as stored, then against the float64 sums of the ideal dy
        dys = dy.cpu().double().view(B, T, D)
        _close_f32(r[2], dys.sum(1), sum_floor * _rms(dys), "dy colsum " + tag)
    assert float(dmod_g[:, :g_o].abs().max()) == 0.0, tag

    # --- the fused pass: LayerNorm backward + the gate backward of the branch in front, on the dx just produced
    def fused():
        dmod_u = torch.zeros(B, mod_ld, device=DEV)
        dx = dres.clone() if dres_mode == "alias" else torch.empty(M, D, device=DEV)
        dres_in = {"none": None, "separate": ptr(dres), "alias": ptr(dx)}[dres_mode]
        dy = torch.empty(M, D, device=DEV, dtype=tdt)
        cp = torch.empty(B, D, device=DEV) if want_cp else None
        ops.check(lib().vaw_ln_modulate_bwd_gate(dt, ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(mod) + 4 * sc_o, mod_ld, dres_in, ptr(dx),
                                                 ptr(dmod_u) + 4 * sh_o, ptr(dmod_u) + 4 * sc_o, mod_ld, ptr(y), ptr(mod) + 4 * gn_o, ptr(dy),
                                                 ptr(dmod_u) + 4 * gn_o, ptr(cp) if want_cp else None, B, T, D, *_wsargs(ws), stream_ptr()),
                  "vaw_ln_modulate_bwd_gate")
        torch.cuda.synchronize()
        return (dx, dmod_u, dy) + ((cp,) if want_cp else ())
    r = _twice(fused)
    dx_u, dmod_u, dy_u = r[0], r[1], r[2]
    _close_f32(dx_u, ref_dx, 1e-5 * _rms(ref_dx), "fused dx " + tag)
    _close_f32(dmod_u[:, sh_o:sh_o + D], ref_dsh, sum_floor * _rms(dxh), "fused dshift " + tag)
    _close_f32(dmod_u[:, sc_o:sc_o + D], ref_dsc, sum_floor * _rms(dxh.reshape(M, D) * xh), "fused dscale " + tag)
    ref_dyn = (ref_dx.view(B, T, D) * gate_n[:, None]).reshape(M, D)
    _close_out(dt, dy_u, ref_dyn, 1e-5 * _rms(ref_dyn), "fused dy " + tag)
    terms = ref_dx.view(B, T, D) * y_h.double().view(B, T, D)
    _close_f32(dmod_u[:, gn_o:gn_o + D], terms.sum(1), sum_floor * _rms(terms), "fused dgate " + tag)
    if want_cp:
        dys = dy_u.cpu().double().view(B, T, D)
        _close_f32(r[3], dys.sum(1), sum_floor * _rms(dys), "fused dy colsum " + tag)
    if D <= 1280:      # bitwise the pair: vaw_ln_modulate_bwd, then vaw_gate_bwd on its dx
        assert torch.equal(dx_u, dx) and torch.equal(dmod_u[:, sh_o:sc_o + D], dmod[:, sh_o:sc_o + D]), tag
        dmod_p = torch.zeros(B, mod_ld, device=DEV)
        dy_p = torch.empty(M, D, device=DEV, dtype=tdt)
        cp_p = torch.empty(B, D, device=DEV)
        ops.check(lib().vaw_gate_bwd(dt, ptr(dx), ptr(y), ptr(mod) + 4 * gn_o, mod_ld, ptr(dy_p), ptr(dmod_p) + 4 * gn_o, mod_ld,
                                     ptr(cp_p), B, T, D, *_wsargs(ws), stream_ptr()), "vaw_gate_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dy_u, dy_p) and torch.equal(dmod_u[:, gn_o:gn_o + D], dmod_p[:, gn_o:gn_o + D]), tag
        if want_cp:
            assert torch.equal(r[3], cp_p), tag


def _quantise(src_bf16, fmt, scale0):
    """what vaw_fp8_quantize_delayed makes of a bf16 tensor: (bytes, running max)"""
    R, C = src_bf16.shape
    st = ops.fp8_states([fmt], torch.device(DEV))
    st[:, 0] = scale0
    q = torch.empty(R, C, device=DEV, dtype=torch.uint8)
    ops.check(lib().vaw_fp8_quantize_delayed(BF16, fmt, ptr(src_bf16), R, C, C, ptr(q), C, None, 0, ptr(st), stream_ptr()),
              "vaw_fp8_quantize_delayed")
    torch.cuda.synchronize()
    return q, st[0, 1].clone()


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("fmt", list(FMT))
def test_fp8_row_kernels_are_the_quantised_bf16_kernels(fmt, D, regime):
    """vaw_ln_modulate_fwd_fp8, vaw_gate_bwd_fp8 and vaw_ln_modulate_bwd_gate_fp8: the bytes and the running max equal what the
    quantiser makes of the bf16 entry point's output with the same scale, every f32 side output is bitwise the bf16 entry point's
    (those are checked against float64 in test_row_kernels_vs_float64 on the same inputs), and two runs are bitwise equal."""
    code = FMT[fmt]
    B, T, use_ws = REGIMES[regime]
    M = B * T
    mod_ld, base, dres_mode, want_cp = _case(D, regime)
    h = _data(B, T, D, mod_ld, seed=D * 7 + T)
    x, mod, dout, dres, y = h["x"].to(DEV), h["mod"].to(DEV), h["dout"].bfloat16().to(DEV), h["dres"].to(DEV), h["y"].bfloat16().to(DEV)
    sh_o, sc_o, g_o, gn_o = base + 3 * D, base + 4 * D, base + 5 * D, base + 2 * D
    ws = ops._row_ws(B, T, D) if use_ws else None
    tag = f"{fmt} D={D} {regime} mod_ld={mod_ld} dres={dres_mode} cp={want_cp}"
    scale0 = 0.02
    p_f = _plan(L.ROW_LN_FWD_FP8, BF16, B, T, D, ws)
    assert p_f.variant == L.RV_LN_FWD and p_f.nv == _nv(D) and p_f.grid_x <= 2048
    p_g, p_u = _plan(L.ROW_GATE_BWD_FP8, BF16, B, T, D, ws), _plan(L.ROW_LN_BWD_GATE_FP8, BF16, B, T, D, ws)
    fits = (2 + 4 * (p_u.block // 64)) * D * 4 <= 160 * 1024
    assert p_g.variant == L.RV_ROW_GATE and p_u.variant == (L.RV_ROW_FUSE8 if _nv(D) <= 5 and fits else L.RV_ROW_FUSE), tag
    for p in (p_g, p_u):
        _check_split(p, regime, B, T, D, tag)

    def state():
        st = ops.fp8_states([code], torch.device(DEV))
        st[:, 0] = scale0
        return st

    # --- forward
    out = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.check(lib().vaw_ln_modulate_fwd(BF16, ptr(x), ptr(mod) + 4 * sh_o, ptr(mod) + 4 * sc_o, mod_ld, ptr(out), ptr(mean), ptr(rstd),
                                        B, T, D, EPS, stream_ptr()), "vaw_ln_modulate_fwd")

    def fwd8():
        q, st = torch.empty(M, D, device=DEV, dtype=torch.uint8), state()
        m2, r2 = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        ops.check(lib().vaw_ln_modulate_fwd_fp8(ptr(x), ptr(mod) + 4 * sh_o, ptr(mod) + 4 * sc_o, mod_ld, ptr(q), ptr(st), code, ptr(m2),
                                                ptr(r2), B, T, D, EPS, stream_ptr()), "vaw_ln_modulate_fwd_fp8")
        torch.cuda.synchronize()
        return q, st, m2, r2
    q, st, m2, r2 = _twice(fwd8)
    q_ref, amax = _quantise(out, code, scale0)
    assert torch.equal(q, q_ref) and float(st[0, 1]) == float(amax) == float(out.float().abs().max()), "fwd " + tag
    assert torch.equal(m2, mean) and torch.equal(r2, rstd), "fwd " + tag

    # --- gate backward
    dy = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
    dmod_g, cp_g = torch.zeros(B, mod_ld, device=DEV), torch.empty(B, D, device=DEV)
    ops.check(lib().vaw_gate_bwd(BF16, ptr(dres), ptr(y), ptr(mod) + 4 * g_o, mod_ld, ptr(dy), ptr(dmod_g) + 4 * g_o, mod_ld, ptr(cp_g),
                                 B, T, D, *_wsargs(ws), stream_ptr()), "vaw_gate_bwd")

    def gate8():
        q, st = torch.empty(M, D, device=DEV, dtype=torch.uint8), state()
        dmod8, cp8 = torch.zeros(B, mod_ld, device=DEV), torch.empty(B, D, device=DEV)
        ops.check(lib().vaw_gate_bwd_fp8(ptr(dres), ptr(y), ptr(mod) + 4 * g_o, mod_ld, ptr(q), ptr(st), code, ptr(dmod8) + 4 * g_o, mod_ld,
                                         ptr(cp8) if want_cp else None, B, T, D, *_wsargs(ws), stream_ptr()), "vaw_gate_bwd_fp8")
        torch.cuda.synchronize()
        return q, st, dmod8, cp8 if want_cp else cp_g
    q, st, dmod8, cp8 = _twice(gate8)
    q_ref, amax = _quantise(dy, code, scale0)
    assert torch.equal(q, q_ref) and float(st[0, 1]) == float(amax), "gate " + tag
    assert torch.equal(dmod8, dmod_g) and torch.equal(cp8, cp_g), "gate " + tag

    # --- the fused pass
    def fused(q8):
        dmod_u = torch.zeros(B, mod_ld, device=DEV)
        dx = dres.clone() if dres_mode == "alias" else torch.empty(M, D, device=DEV)
        dres_in = {"none": None, "separate": ptr(dres), "alias": ptr(dx)}[dres_mode]
        cp = torch.empty(B, D, device=DEV)
        common = (ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(mod) + 4 * sc_o, mod_ld, dres_in, ptr(dx), ptr(dmod_u) + 4 * sh_o,
                  ptr(dmod_u) + 4 * sc_o, mod_ld, ptr(y), ptr(mod) + 4 * gn_o)
        if q8:
            dyq, st = torch.empty(M, D, device=DEV, dtype=torch.uint8), state()
            ops.check(lib().vaw_ln_modulate_bwd_gate_fp8(*common, ptr(dyq), ptr(st), code, ptr(dmod_u) + 4 * gn_o,
                                                         ptr(cp) if want_cp else None, B, T, D, *_wsargs(ws), stream_ptr()),
                      "vaw_ln_modulate_bwd_gate_fp8")
        else:
            dyq, st = torch.empty(M, D, device=DEV, dtype=torch.bfloat16), state()
            ops.check(lib().vaw_ln_modulate_bwd_gate(BF16, *common, ptr(dyq), ptr(dmod_u) + 4 * gn_o, ptr(cp) if want_cp else None,
                                                     B, T, D, *_wsargs(ws), stream_ptr()), "vaw_ln_modulate_bwd_gate")
        torch.cuda.synchronize()
        return dx, dmod_u, dyq, st, cp if want_cp else dx[:0]
    dx_b, dmod_b, dy_b, _, cp_b = fused(False)
    dx8, dmod8, q, st, cp8 = _twice(lambda: fused(True))
    q_ref, amax = _quantise(dy_b, code, scale0)
    assert torch.equal(q, q_ref) and float(st[0, 1]) == float(amax), "fused " + tag
    assert torch.equal(dx8, dx_b) and torch.equal(dmod8, dmod_b) and torch.equal(cp8, cp_b), "fused " + tag


# ------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("path", ["bf16x8", "vec4_f32", "vec4_bf16", "scalar_f32", "scalar_bf16"])
def test_colsum_each_path_vs_float64(path, beta):
    """vaw_colsum as dit.py calls it for the adaLN bias (a column block of the dmod rows: ldx > N, base offset into the row) and on
    whole tensors, M off the 128- and 512-row blocks; each path asserted through the plan."""
    # (dtype, M, N, ldx, element offset of the base, path)
    D = 96
    case = {"bf16x8": (BF16, 1100, 264, 8 * D, 8 * 3, L.RV_COLSUM_BF16X8),
            "vec4_f32": (F32, 1100, 260, 14 * D, 4 * 6, L.RV_COLSUM_VEC4),
            "vec4_bf16": (BF16, 700, 264, 8 * D, 8, L.RV_COLSUM_VEC4),          # M < 1024: the 512-row kernel
            "scalar_f32": (F32, 1300, 259, 14 * D, 3, L.RV_COLSUM_SCALAR),
            "scalar_bf16": (BF16, 515, 7, 9, 1, L.RV_COLSUM_SCALAR)}[path]
    dt, M, N, ldx, off, variant = case
    tdt = TORCH_DT[dt]
    es = 4 if dt == F32 else 2
    g = torch.Generator().manual_seed(M + N)
    buf_h = (torch.randn(M, ldx, generator=g) * 3 + 0.25).to(tdt)
    buf = buf_h.to(DEV)
    X = ptr(buf) + es * off
    p = ops.row_plan(L.ROW_COLSUM, dt, M, 1, N, ldx=ldx, base_addr=X)
    assert p.variant == variant and M % p.rows_per_chunk != 0, path
    ref = buf_h.double()[:, off:off + N].sum(0)
    out0 = torch.randn(N, generator=g)
    out = out0.to(DEV)
    ops.colsum(dt, X, M, N, ldx, ptr(out), beta)
    torch.cuda.synchronize()
    terms = buf_h.double()[:, off:off + N]
    _close_f32(out, ref + beta * out0.double(), 1e-5 * math.sqrt(M) * _rms(terms), f"colsum {path}")
    out2 = out0.to(DEV)
    ops.colsum(dt, X, M, N, ldx, ptr(out2), beta)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


# ------------------------------------------------------------------------------------------------
# model level: hidden 1280 (the LDS-limit width of the fused pass)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dit_hidden_1280_vs_oracle(dtype):
    """vaw_amd.DiT(hidden_size=1280) forward + backward against oracle.dit with the same weights; fp32 at the tiny-DiT golden
    tolerances, bf16 at the tiny-DiT bf16 ones (test_gpu_dit.py)."""
    from oracle import dit as odit
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=1280, depth=1, num_heads=20, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=False)
    torch.manual_seed(5)
    om = odit.DiT(**kw)
    perturb_(om, 31)
    hm = vaw_amd.DiT(compute_dtype=dtype, **kw)
    hm.load_state_dict(om.state_dict())
    hm = hm.to(DEV).train()
    om.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 4, 8, 8, generator=g)
    t = torch.tensor([17.0, 803.0])
    y = torch.tensor([3, 8])
    gout = torch.randn(2, 4, 8, 8, generator=g)
    if dtype == "bf16":       # whole tensors: the float64 oracle and its own bf16-autocast distance from it (tests/model_grad_cases.py)
        g64, e_ref = grad_cases.oracle_yardstick("dit", om, x, t, y, gout)
    om = om.double()          # the oracle in float64 (its timestep embedding is f32 by construction: fed to the MLP as f64)
    om.t_embedder.mlp.register_forward_pre_hook(lambda mod, a: (a[0].double(),))
    xo = x.double().requires_grad_(True)
    ref, _ = om(xo, t, y)
    (ref * gout.double()).sum().backward()
    xh = x.to(DEV).requires_grad_(True)
    out, _ = hm(xh, t.to(DEV), y.to(DEV))
    (out * gout.to(DEV)).sum().backward()
    ref, gx = ref.detach().float(), xo.grad.float()
    grads = {k: p.grad.float() for k, p in om.named_parameters() if p.grad is not None}
    assert float(ref.abs().max()) > 1e-3 and len(grads) == len([p for p in hm.parameters() if p.grad is not None])
    if dtype == "fp32":
        # twice the tiny-DiT golden tolerances, in units of each tensor's rms: at K = 1280 the HIP fp32 path differs from float64 by up
        # to 5e-5 x rms in dx and 1.2e-4 x rms in the patch-embedding weight gradient (measured; the row kernels on their own are held
        # to 1e-5 by test_row_kernels_vs_float64, so the excess comes from elsewhere in the model and is not this test's subject)
        torch.testing.assert_close(out.detach().cpu(), ref, rtol=1e-4, atol=1e-4 * _rms(ref))
        torch.testing.assert_close(xh.grad.cpu(), gx, rtol=1e-4, atol=1e-4 * _rms(gx))
        golden = {}
        for k, v in grads.items():
            stats, sample = fingerprint(v)
            golden[k] = {"stats": stats, "sample": sample}
        assert_fingerprints({k: p.grad.cpu() for k, p in hm.named_parameters() if k in grads}, golden, 2e-4, 2e-5, "gradients")
    else:
        assert float((out.detach().cpu() - ref).norm() / ref.norm()) < 3e-2
        assert float((xh.grad.cpu() - gx).norm() / gx.norm()) < 5e-2
        for k, p in hm.named_parameters():
            if k in grads:
                gl2 = float(grads[k].double().norm())
                assert abs(float(p.grad.double().norm()) - gl2) <= 5e-2 * gl2 + 1e-4, k
        # ... and what a norm does not see (a swapped, permuted, transposed or sign-flipped gradient): every tensor within twice the
        # oracle's bf16 distance from float64
        got = {k: p.grad for k, p in hm.named_parameters() if k in grads}
        got.update({grad_cases.OUT: out.detach(), grad_cases.GX: xh.grad})
        worst, n = grad_cases.hold_whole_tensors(got, g64, e_ref)
        assert n == len(g64) == len(grads) + 2
        print(f"\nDiT hidden 1280 bf16: worst rel_err / e_ref {worst[0]:.3f} at {worst[1]} ({worst[2]:.5f} / {worst[3]:.5f})")


def test_dit_hidden_1280_fp8_fused_rows_are_bitwise_the_pair():
    """fp8 mode, hidden 1280: four delayed-scaling steps with the fused LayerNorm-backward + gate-backward pass
    (vaw_ln_modulate_bwd_gate_fp8 at D = 1280, the register form: its LDS-slab form does not fit) and with the pair of kernels;
    losses and parameters bitwise equal (both write the same bf16 roundings as fp8 bytes)."""
    import random

    import numpy as np

    def run(fuse_rows):
        random.seed(3); np.random.seed(3); torch.manual_seed(3)
        m = vaw_amd.DiT(image_size=16, patch_size=2, in_channels=4, hidden_size=1280, depth=1, num_heads=20, class_dropout_prob=0.0,
                        num_classes=10, compute_dtype="fp8")
        m.fp8_fuse_rows = fuse_rows
        perturb_(m, 7, std=0.02)
        m = m.to(DEV).train()
        opt = vaw_amd.FusedAdamW(m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
        from conftest import base_args
        diff = vaw_amd.GaussianDiffusion(args=base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=16),
                                         betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                         model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                         loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        g = torch.Generator().manual_seed(1)
        x0 = (torch.randn(2, 4, 16, 16, generator=g) * 0.5).to(DEV)
        noise = torch.randn(2, 4, 16, 16, generator=g).to(DEV)
        t = torch.randint(0, 1000, (2,), generator=g).to(DEV)
        y = torch.randint(0, 10, (2,), generator=g).to(DEV)
        losses = []
        for _ in range(4):
            opt.zero_grad()
            terms = diff.training_losses(m, x0, None, t=t, model_kwargs={"y": y}, noise=noise)
            terms["loss"].mean().backward()
            opt.step()
            losses.append(terms["mse"].detach().cpu())
        assert m._ws_cur.fp8 and m._ws_cur.d_bwd
        return torch.stack(losses), m._flat.detach().cpu().clone()
    (la, pa), (lb, pb) = run(True), run(False)
    assert torch.isfinite(la).all() and torch.equal(la, lb) and torch.equal(pa, pb)

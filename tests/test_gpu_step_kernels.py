"""Direct float64 parity of the objective kernels and the DiT conditioning / patch kernels of csrc/elementwise.hip and of the
vaw_reduce_rows fold of csrc/layernorm.hip, at the smallest shapes that reach each of their paths: the scalar tail, the second block
along a row, the grid-stride second trip, the second column trip of the embedding scatter, the unrolled loop's remainder of the cast with
column sums, every branch of the variational bound.

References, allowances and comparators are those of tests/step_parity.py (checked on the CPU by test_step_kernels_cpu.py); every test
names its kind: exact (torch.equal / equal bits), derived bound (roundings counted from the kernel, no margin) or transcendental
(vaw_silu_fwd / vaw_silu_bwd / vaw_silu_bwd_cast, vaw_timestep_embedding, vaw_vb_fwd / vaw_vb_bwd).  Outputs are NaN-filled before the
call and carry a 64-element canary tail that must come back intact.  Run on the MI355X box: pytest -m gpu (-s prints the worst
error / allowance of every bounded case)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_parity as sp
from step_parity import NAN, U, same_bits, within
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, lib, ptr, stream_ptr

DEV = "cuda"
T = sp.T_STEPS
f32 = np.float32


def _dt(dtype):
    return F32 if dtype == torch.float32 else BF16


def _ok(rc):
    assert rc == 0, (rc, lib().vaw_last_error_string().decode())
    torch.cuda.synchronize()


def _buf(n, dtype=torch.float32, fill=NAN, off=0):
    """`off` canary elements, n elements of `fill`, the canary tail; off = 1 puts an f32 payload one float past a 16-byte boundary"""
    b = sp.guarded(off + n, dtype, NAN, DEV)
    b[off:off + n] = fill.reshape(-1).to(DEV) if isinstance(fill, torch.Tensor) else fill
    if off:
        b[:off] = sp.CANARY
    return b


def _p(buf, off=0):
    return ptr(buf) + off * buf.element_size()


def _intact(buf, n, off=0):
    return sp.tail_intact(buf, off + n) and bool((buf[:off] == sp.CANARY).all())


def _got(buf, n, off=0):
    return buf[off:off + n].cpu()


def _note(kernel, case, ratio):
    print(f"RATIO {kernel} {case}: max err / allowance = {ratio:.4f}")


def _check(kernel, case, got, ref, allow, exact):
    """exact: the f32 result equals the float64 reference; otherwise the derived bound / transcendental allowance, no margin"""
    if exact:
        bad = (got.double() != ref).nonzero()
        assert torch.equal(got.double(), ref), f"{kernel} {case}: {bad.shape[0]} of {ref.numel()} differ, first at {bad[0].tolist()}"
        return
    ok, ratio = within(got, ref, allow)
    _note(kernel, case, ratio)
    assert ok, f"{kernel} {case}: max err / allowance = {ratio}"


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. row streams: vaw_qsample_fwd, vaw_mix_rows, vaw_wmse_bwd, vaw_wmse_bwd_t, vaw_latent_qsample
#    n = 1, 3: the scalar loop alone; 4: one vector; 75: scalar, one block; 1024 / 1028: the second block of a row, vectors;
#    65540: 16385 vectors, one more than 64 blocks x 256 threads take in a trip; 65543: the same trip structure on the scalar loop
# ------------------------------------------------------------------------------------------------------------------------------------
ROW_N = [1, 3, 4, 75, 1024, 1028, 65540, 65543]
KINDS = ["integer", "random"]


@functools.lru_cache(maxsize=None)
def _mse_case(B, n, integer):
    c = sp.mse_case(B, n, integer)
    c["t"] = sp.timesteps(B)
    return c


def _dev(c, off=0, keys=("out", "x0", "noise")):
    d = {k: _buf(c[k].numel(), fill=c[k], off=off) for k in keys}
    d.update({k: c[k].to(DEV) for k in ("ca", "cb", "w")})
    return d


def _qsample(c, d, t, B, n, off=0):
    xt = _buf(B * n, off=off)
    _ok(lib().vaw_qsample_fwd(_p(d["x0"], off), _p(d["noise"], off), ptr(t), ptr(d["ca"]), ptr(d["cb"]), T, _p(xt, off), B, n, stream_ptr()))
    assert _intact(xt, B * n, off)
    return _got(xt, B * n, off).view(B, n)


def _mix(c, d, a, cc, B, n, off=0):
    o = _buf(B * n, off=off)
    _ok(lib().vaw_mix_rows(_p(d["x0"], off), _p(d["noise"], off), ptr(a), ptr(cc), _p(o, off), B, n, stream_ptr()))
    assert _intact(o, B * n, off)
    return _got(o, B * n, off).view(B, n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", ROW_N)
def test_qsample_and_mix_rows(n, B, kind):
    """integer: exact (power-of-two tables, data in [-2, 2]: |a x + c y| <= 8, every product and the sum exact).  random: derived
    bound 3 u (|a x| + |c y|) (mix_ref).  Timesteps 0 and T - 1 included; vaw_mix_rows with the gathered rows is the same bits."""
    c = _mse_case(B, n, kind == "integer")
    d, t = _dev(c), c["t"].to(DEV)
    ref, allow = sp.qsample_ref(c["x0"], c["noise"], c["t"], c["ca"], c["cb"])
    got = _qsample(c, d, t, B, n)
    _check("vaw_qsample_fwd", f"{B}x{n} {kind}", got, ref, allow, kind == "integer")
    got2 = _mix(c, d, c["ca"][c["t"]].to(DEV), c["cb"][c["t"]].to(DEV), B, n)
    assert same_bits(got, got2)
    assert _intact(d["x0"], B * n) and same_bits(_got(d["x0"], B * n).view(B, n), c["x0"])


def _wmse_bwd_calls(c, d, B, n, integer, off=0):
    """the three ways into wmse_bwd_t_kernel: (entry, got, ref, allowance)"""
    t = c["t"]
    a, cc, w = c["ca"][t], c["cb"][t], c["w"][t]
    if integer:           # gm = n 2^j: k = gm w 2 / n is a power of two and exact, the bracket a multiple of 0.5 below 10
        g_row = float(n) * 2.0 ** (torch.arange(B) % 3 - 1).float()
        g_one, inv = torch.tensor([float(n)]), 0.25
    else:
        gg = sp.gen(B, n, 5)
        g_row, g_one, inv = torch.rand(B, generator=gg) + 0.5, torch.rand(1, generator=gg) + 0.5, 1.0 / (3 * B)
    res = []
    av, cv, wv, td, grd, god = a.to(DEV), cc.to(DEV), w.to(DEV), t.to(DEV), g_row.to(DEV), g_one.to(DEV)     # alive across the launches
    args = (_p(d["out"], off), _p(d["x0"], off), _p(d["noise"], off))
    ref_row, unit_row = sp.wmse_grad_ref(c["out"], c["x0"], c["noise"], a, cc, w, g_row)
    gm = (g_one.double() * float(f32(inv))).expand(B)
    ref_one, unit_one = sp.wmse_grad_ref(c["out"], c["x0"], c["noise"], a, cc, w, gm)
    for name in ("vaw_wmse_bwd", "vaw_wmse_bwd_t", "vaw_wmse_bwd_t/rows"):
        o = _buf(B * n, off=off)
        if name == "vaw_wmse_bwd":
            _ok(lib().vaw_wmse_bwd(*args, ptr(av), ptr(cv), ptr(wv), ptr(grd), _p(o, off), B, n, stream_ptr()))
            ref, allow = ref_row, 7 * unit_row
        elif name == "vaw_wmse_bwd_t":
            _ok(lib().vaw_wmse_bwd_t(*args, ptr(td), ptr(d["ca"]), ptr(d["cb"]), ptr(d["w"]), T, ptr(god), inv,
                                     _p(o, off), B, n, stream_ptr()))
            ref, allow = ref_one, 8 * unit_one
        else:             # t = NULL: the per-row vectors with the scalar gradient
            _ok(lib().vaw_wmse_bwd_t(*args, None, ptr(av), ptr(cv), ptr(wv), 0, ptr(god), inv, _p(o, off), B, n, stream_ptr()))
            ref, allow = ref_one, 8 * unit_one
        assert _intact(o, B * n, off), name
        res.append((name, _got(o, B * n, off).view(B, n), ref, allow))
    return res


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", ROW_N)
def test_wmse_bwd_both_forms(n, B, kind):
    """integer: exact.  random: derived bound, 7 roundings in the per-row form g[b] and 8 in the scalar form g * inv_count
    (wmse_grad_ref), each at most u |k| (|o| + |a x| + |c nz|)."""
    c = _mse_case(B, n, kind == "integer")
    for name, got, ref, allow in _wmse_bwd_calls(c, _dev(c), B, n, kind == "integer"):
        _check(name, f"{B}x{n} {kind}", got, ref, allow, kind == "integer")


def _latent_case(B, n, integer):
    g = sp.gen(B, n, int(integer), 211)
    c = _mse_case(B, n, integer)
    if integer:
        lat, eps = sp.ints(g, B, 2, n).float(), sp.ints(g, B, n).float()
        return lat, eps, 0.5, 0.25            # (m + s e) / 2: multiples of 0.5 below 3.5; the mix of it a multiple of 0.25 below 11
    return torch.randn(B, 2, n, generator=g), torch.randn(B, n, generator=g), 0.18215, 1000.0 / T * 0.37


def _latent_qsample(c, lat, eps, t, scale, ts, B, n):
    bl, be, bn = _buf(2 * B * n, fill=lat), _buf(B * n, fill=eps), _buf(B * n, fill=c["noise"])
    x0, xt, tf = _buf(B * n), _buf(B * n), _buf(B)
    td, ca, cb = t.to(DEV), c["ca"].to(DEV), c["cb"].to(DEV)
    _ok(lib().vaw_latent_qsample(ptr(bl), ptr(be), ptr(bn), ptr(td), ptr(ca), ptr(cb), T, scale, ts,
                                 ptr(x0), ptr(xt), ptr(tf), B, n, stream_ptr()))
    assert _intact(x0, B * n) and _intact(xt, B * n) and _intact(tf, B)
    return _got(x0, B * n).view(B, n), _got(xt, B * n).view(B, n), _got(tf, B)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", ROW_N)
def test_latent_qsample(n, B, kind):
    """integer: exact.  random: derived bound of latent_qsample_ref (3 roundings into x0, those carried and 3 more into x_t);
    tf = float(t) * t_scale is one product: exact kind, bitwise the f32 product."""
    integer = kind == "integer"
    c = _mse_case(B, n, integer)
    lat, eps, scale, ts = _latent_case(B, n, integer)
    x0, xt, tf = _latent_qsample(c, lat, eps, c["t"], scale, ts, B, n)
    r0, a0, rt, at, rtf = sp.latent_qsample_ref(lat, eps, c["noise"], c["t"], c["ca"], c["cb"], scale, ts)
    _check("vaw_latent_qsample x0", f"{B}x{n} {kind}", x0, r0, a0, integer)
    _check("vaw_latent_qsample x_t", f"{B}x{n} {kind}", xt, rt, at, integer)
    assert same_bits(tf, rtf.float())


@pytest.mark.parametrize("n", [75, 1028])
def test_out_of_range_timesteps_poison_their_rows_only(n):
    """exact: t = -1 and t = T give rows of NaN (and a NaN loss), rows 0 and 3 (t = 0, T - 1) are what the integer case gives."""
    B = 4
    c = dict(sp.mse_case(B, n, True, seed=9))
    t = torch.tensor([0, -1, T, T - 1])
    tv = t.clamp(0, T - 1)
    d, td = _dev(c), t.to(DEV)
    good, bad = torch.tensor([0, 3]), torch.tensor([1, 2])
    ref, _ = sp.qsample_ref(c["x0"], c["noise"], t, c["ca"], c["cb"])
    got = _qsample(c, d, td, B, n)
    assert bool(torch.isnan(got[bad]).all()) and torch.equal(got[good].double(), ref[good])
    lat, eps = sp.ints(sp.gen(n, 213), B, 2, n).float(), sp.ints(sp.gen(n, 215), B, n).float()
    x0, xt, tf = _latent_qsample(c, lat, eps, t, 0.5, 0.25, B, n)
    r0, _, rt, _, rtf = sp.latent_qsample_ref(lat, eps, c["noise"], t, c["ca"], c["cb"], 0.5, 0.25)
    assert bool(torch.isnan(xt[bad]).all()) and torch.equal(xt[good].double(), rt[good]) and torch.equal(x0.double(), r0)
    assert same_bits(tf, rtf.float())
    g_one = torch.tensor([float(n)], device=DEV)
    o = _buf(B * n)
    _ok(lib().vaw_wmse_bwd_t(ptr(d["out"]), ptr(d["x0"]), ptr(d["noise"]), ptr(td), ptr(d["ca"]), ptr(d["cb"]), ptr(d["w"]), T,
                             ptr(g_one), 0.25, ptr(o), B, n, stream_ptr()))
    ref, _ = sp.wmse_grad_ref(c["out"], c["x0"], c["noise"], c["ca"][tv], c["cb"][tv], c["w"][tv], torch.full((B,), 0.25 * n))
    dout = _got(o, B * n).view(B, n)
    assert bool(torch.isnan(dout[bad]).all()) and torch.equal(dout[good].double(), ref[good]) and _intact(o, B * n)
    mse, mean = _buf(B), _buf(1)
    _ok(lib().vaw_wmse_fwd_t(ptr(d["out"]), ptr(d["x0"]), ptr(d["noise"]), ptr(td), ptr(d["ca"]), ptr(d["cb"]), ptr(d["w"]), T,
                             ptr(mse), ptr(mean), 1.0, B, n, stream_ptr()))
    m = _got(mse, B)
    assert bool(torch.isnan(m[bad]).all()) and bool(torch.isfinite(m[good]).all()) and bool(torch.isnan(_got(mean, 1)).all())
    assert _intact(mse, B) and _intact(mean, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. per-sample reductions: vaw_wmse_fwd, vaw_wmse_fwd_t, batch_mean_kernel
#    n = 1, 75: fewer elements than threads; 4096: one vector a thread; 4100: a thread with two vectors; 12292: three trips, ragged
# ------------------------------------------------------------------------------------------------------------------------------------
RED_N = [1, 75, 4096, 4100, 12292]


def _wmse_fwd_calls(c, d, B, n, off=0):
    """the three ways into wmse_fwd_t_kernel: per-row vectors through vaw_wmse_fwd and through vaw_wmse_fwd_t(t = NULL), tables"""
    t = c["t"]
    av, cv, wv = (c[k][t].to(DEV) for k in ("ca", "cb", "w"))
    td = t.to(DEV)
    args = (_p(d["out"], off), _p(d["x0"], off), _p(d["noise"], off))
    outs = []
    for name in ("vaw_wmse_fwd", "vaw_wmse_fwd_t", "vaw_wmse_fwd_t/rows"):
        mse = _buf(B)
        if name == "vaw_wmse_fwd":
            _ok(lib().vaw_wmse_fwd(*args, ptr(av), ptr(cv), ptr(wv), ptr(mse), B, n, stream_ptr()))
        elif name == "vaw_wmse_fwd_t":
            _ok(lib().vaw_wmse_fwd_t(*args, ptr(td), ptr(d["ca"]), ptr(d["cb"]), ptr(d["w"]), T, ptr(mse), None, 1.0, B, n, stream_ptr()))
        else:
            _ok(lib().vaw_wmse_fwd_t(*args, None, ptr(av), ptr(cv), ptr(wv), 0, ptr(mse), None, 1.0, B, n, stream_ptr()))
        assert _intact(mse, B), name
        outs.append((name, _got(mse, B)))
    return outs


def _wmse_exact(c, n):
    """the f32 value of the integer case: the sum of squares is exact (mse_case), tot / n rounds once, w is a power of two"""
    t = c["t"]
    a, cc = c["ca"][t].double()[:, None], c["cb"][t].double()[:, None]
    d = a * c["x0"].double() + cc * c["noise"].double() - c["out"].double()
    sq = (d * d).sum(1).numpy()
    return torch.from_numpy((sq.astype(f32) / f32(n)) * c["w"][t].numpy())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", RED_N)
def test_wmse_fwd_all_entries(n, kind):
    """integer: exact -- the one rounding of tot / n restated in f32.  random: derived bound of wmse_ref (4 roundings into each
    difference, the chain ceil(n / 1024) + 3 + 6 + 16 of the block sum, 2 roundings of the result).  The three entries agree bitwise."""
    B = 3
    c = _mse_case(B, n, kind == "integer")
    outs = _wmse_fwd_calls(c, _dev(c), B, n)
    t = c["t"]
    ref, allow = sp.wmse_ref(c["out"], c["x0"], c["noise"], c["ca"][t], c["cb"][t], c["w"][t])
    for name, got in outs:
        if kind == "integer":
            want = _wmse_exact(c, n)
            assert same_bits(got, want), (name, got.tolist(), want.tolist())
        else:
            _check(name, f"{B}x{n}", got, ref, allow, False)
        assert same_bits(got, outs[0][1]), name


@pytest.mark.parametrize("accum", [1.0, 2.0])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 700])
def test_batch_mean_through_wmse_fwd_t(B, accum):
    """B <= 256: one value a thread; 257 and 700: a thread adds two and three.  exact: rows of n = 4 integers give losses that are
    multiples of 2^-5 below 800, so every partial sum of at most 700 of them is exact and the mean is the two f32 divisions.
    derived bound on random rows (n = 75): batch_mean_ref from the losses the kernel itself wrote."""
    for integer, n in ((True, 4), (False, 75)):
        c = _mse_case(B, n, integer)
        d, td = _dev(c), c["t"].to(DEV)
        mse, mean = _buf(B), _buf(1)
        _ok(lib().vaw_wmse_fwd_t(ptr(d["out"]), ptr(d["x0"]), ptr(d["noise"]), ptr(td), ptr(d["ca"]), ptr(d["cb"]), ptr(d["w"]), T,
                                 ptr(mse), ptr(mean), accum, B, n, stream_ptr()))
        assert _intact(mse, B) and _intact(mean, 1)
        m, got = _got(mse, B), _got(mean, 1)
        if integer:
            assert same_bits(m, _wmse_exact(c, n))
            want = (f32(m.double().sum().item()) / f32(B)) / f32(accum)
            assert float(got) == float(want), (float(got), float(want))
        else:
            ref, allow = sp.batch_mean_ref(m, accum)
            _check("batch_mean_kernel", f"B={B} accum={accum}", got, ref.reshape(1), allow.reshape(1), False)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. vaw_vb_fwd / vaw_vb_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vb_case(n, mm, vm):
    return sp.vb_case(n, mm, vm)


def _vb_dev(c):
    B, n = c["x0"].shape
    d = {k: _buf(B * n, fill=c[k]) for k in ("mean_out", "x0", "xt")}
    d["var_out"] = None if c["var_out"] is None else _buf(B * n, fill=c["var_out"])
    d["coef"], d["gvb"] = c["coef"].to(DEV), c["gvb"].to(DEV)
    return d


# every mode pair at n = 75 (fewer elements than threads) and 4100 (a thread with five); one pair at the other sizes of RED_N
VB_FWD = [(n, mm, vm) for n in (75, 4100) for mm, vm in sp.VB_MODES] + [(n, 0, 2) for n in (1, 4096, 12292)]


@pytest.mark.parametrize("n,mm,vm", VB_FWD)
def test_vb_fwd_every_mode_and_bin(n, mm, vm):
    """transcendental (vaw_vb_fwd): row 0 is the decoder NLL with x0 in all three bins and elements on each 1e-12 floor, rows 1, 2
    the KL; allowance vb_fwd_allow (4 x the f32-on-the-CPU error, or the running bound of expf / tanhf / logf through every element
    plus the summation chain ceil(n / 1024) + 6 + 16)."""
    c = _vb_case(n, mm, vm)
    d, B = _vb_dev(c), 3
    vb = _buf(B)
    _ok(lib().vaw_vb_fwd(ptr(d["mean_out"]), ptr(d["var_out"]), ptr(d["x0"]), ptr(d["xt"]), ptr(d["coef"]), mm, vm, c["scale"], ptr(vb),
                         B, n, stream_ptr()))
    args = (c["mean_out"], c["var_out"], c["x0"], c["xt"], c["coef"], mm, vm, c["scale"])
    allow, _ = sp.vb_fwd_allow(*args)
    _check("vaw_vb_fwd", f"n={n} mean_mode={mm} var_mode={vm}", _got(vb, B), sp.vb_ref(*args), allow, False)
    assert _intact(vb, B)


VB_BWD = [(mm, vm, which) for mm, vm in sp.VB_MODES for which in (("mean",) if vm == 0 else ("mean", "var", "both"))]


@pytest.mark.parametrize("n", [75, 4100])
@pytest.mark.parametrize("mm,vm,which", VB_BWD)
def test_vb_bwd_every_mode_and_output(n, mm, vm, which):
    """transcendental (vaw_vb_bwd): the kernel's analytic gradients against float64 autograd of the restated value, allowance
    vb_bwd_allow; on the 1e-12 floors the gradient is zero, exactly.  d_mean only, d_var only, both (a fixed variance has no d_var)."""
    c = _vb_case(n, mm, vm)
    d, B = _vb_dev(c), 3
    dm = _buf(B * n) if which in ("mean", "both") else None
    dv = _buf(B * n) if which in ("var", "both") else None
    _ok(lib().vaw_vb_bwd(ptr(d["mean_out"]), ptr(d["var_out"]), ptr(d["x0"]), ptr(d["xt"]), ptr(d["coef"]), mm, vm, c["scale"],
                         ptr(d["gvb"]), ptr(dm), ptr(dv), B, n, stream_ptr()))
    (rm, am), (rv, av) = sp.vb_bwd_allow(c["mean_out"], c["var_out"], c["x0"], c["xt"], c["coef"], mm, vm, c["scale"], c["gvb"])
    for name, buf, ref, allow in (("d_mean", dm, rm, am), ("d_var", dv, rv, av)):
        if buf is None:
            continue
        got = _got(buf, B * n).view(B, n)
        _check("vaw_vb_bwd " + name, f"n={n} mean_mode={mm} var_mode={vm} {which}", got, ref, allow, False)
        assert bool((got[0, c["floors"]] == 0).all()), f"{name}: the gradient on a floor is zero"
        assert _intact(buf, B * n)


@pytest.mark.parametrize("n", RED_N)
@pytest.mark.parametrize("mm,vm", [(0, 0), (1, 1), (0, 2)])
def test_vb_exact_kl_rows(n, mm, vm):
    """exact: log variances 0 (expf(0) = 1) and a model mean d = b + 1 off the true one on even-integer data: every element of row b
    is 0.5 d^2, the row sum 0.5 d^2 n < 2^24 and tot / n are exact; vb = scale * (0.5 d^2 / ln2_f32) and g = gvb * scale /
    (n * ln2_f32) are restated in f32; d_mean = g * d * c2 c1 and d_var = g * (-0.5 d^2) * dlv/dv with power-of-two factors."""
    B = 3
    g = sp.gen(n, mm, vm, 301)
    x0, xt = 2 * sp.ints(g, B, n), 2 * sp.ints(g, B, n)
    coef = torch.zeros(B, sp.SS_NCOEF)
    coef[:, 0], coef[:, 1], coef[:, 2], coef[:, 3] = 1.0, 2.0, 0.5, 1.0          # pred = xt + 2 m; mean = pred / 2 + xt; true = x0 / 2 + xt
    dist = torch.arange(1, B + 1).double()[:, None]
    true_mean = 0.5 * x0 + xt
    mean = true_mean + dist                                                        # d = true - mean = -(b + 1)
    m = mean if mm == 1 else (2.0 * (mean - xt) - xt) / 2.0
    var = None if vm == 0 else torch.zeros(B, n)
    if vm == 2:
        coef[:, 4], coef[:, 5] = 0.0, 0.0
    c = dict(mean_out=m.float(), x0=x0.float(), xt=xt.float(), var_out=var, coef=coef, gvb=torch.tensor([1.0, 0.5, 2.0]))
    d = _vb_dev(c)
    scale = 0.5
    vb, dm, dv = _buf(B), _buf(B * n), (_buf(B * n) if vm else None)
    _ok(lib().vaw_vb_fwd(ptr(d["mean_out"]), ptr(d["var_out"]), ptr(d["x0"]), ptr(d["xt"]), ptr(d["coef"]), mm, vm, scale, ptr(vb), B, n,
                         stream_ptr()))
    _ok(lib().vaw_vb_bwd(ptr(d["mean_out"]), ptr(d["var_out"]), ptr(d["x0"]), ptr(d["xt"]), ptr(d["coef"]), mm, vm, scale, ptr(d["gvb"]),
                         ptr(dm), ptr(dv), B, n, stream_ptr()))
    ln2 = f32(sp.LN2)
    val = (0.5 * dist[:, 0] ** 2).numpy().astype(f32)
    assert same_bits(_got(vb, B), torch.from_numpy(f32(scale) * (val / ln2)))
    gk = (c["gvb"].numpy() * f32(scale)) / (f32(n) * ln2)
    want_dm = torch.from_numpy(gk * dist[:, 0].numpy().astype(f32))[:, None].expand(B, n)     # -d e2 = b + 1; c2 c1 = 1
    assert same_bits(_got(dm, B * n).view(B, n), want_dm.contiguous())
    if vm:
        want_dv = torch.from_numpy(gk * (-val))[:, None].expand(B, n)               # 0.5 (1 - 1 - d^2); dlv/dv = 1, or (c5 - c4) / 2 = 0
        want_dv = want_dv * 0.0 if vm == 2 else want_dv
        assert torch.equal(_got(dv, B * n).view(B, n), want_dv.contiguous())
    assert _intact(vb, B) and _intact(dm, B * n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. vaw_timestep_embedding
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dim", [(b, d) for d in (1, 2, 33, 64, 257) for b in (1, 3)] + [(2049, 257)])
def test_timestep_embedding(B, dim):
    """transcendental (vaw_timestep_embedding): allowance timestep_embedding_ref.  exact: the row of t = 0 is cos 1 | sin 0, the last
    column of an odd dim is zero, and the bf16 output is bitwise the f32 output rounded to nearest even.  2049 x 257 = 526593
    elements: two more blocks' worth than the 2048 x 256 grid covers in one trip."""
    t = torch.tensor([0.0, 0.5, 999.0])
    t = t[2:] if B == 1 else torch.cat([t, torch.rand(B - 3, generator=sp.gen(B, dim)) * 1000.0])
    td = t.to(DEV)
    out = _buf(B * dim)
    _ok(lib().vaw_timestep_embedding(F32, ptr(td), ptr(out), B, dim, 10000.0, stream_ptr()))
    got = _got(out, B * dim).view(B, dim)
    ref, allow = sp.timestep_embedding_ref(t, dim)
    _check("vaw_timestep_embedding", f"{B}x{dim}", got, ref, allow, False)
    half = dim // 2
    if B > 1:
        assert bool((got[0, :half] == 1).all()) and bool((got[0, half:] == 0).all())
    if dim % 2:
        assert bool((got[:, -1] == 0).all())
    ob = _buf(B * dim, torch.bfloat16)
    _ok(lib().vaw_timestep_embedding(BF16, ptr(td), ptr(ob), B, dim, 10000.0, stream_ptr()))
    assert same_bits(_got(ob, B * dim).view(B, dim), sp.bf16_rne(got))
    assert _intact(out, B * dim) and _intact(ob, B * dim)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. SiLU
# ------------------------------------------------------------------------------------------------------------------------------------
SILU_FIXED = [0.0, 1e-6, -1e-6, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0]


@pytest.mark.parametrize("n", [1, 255, 257, 524291])
def test_silu_forward_and_both_backwards(n):
    """transcendental (vaw_silu_fwd, vaw_silu_bwd, vaw_silu_bwd_cast): x ~ N(0, 3) with the fixed points at the end of the vector (in
    the second trip of the 2048 x 256 grid for n = 524291); allowance silu_ref.  At the fixed points the results are finite and carry
    the reference's sign (dy = 1 there).  exact: x = 0 gives 0 and dy / 2; vaw_silu_bwd_cast's dx is bitwise vaw_silu_bwd's and its
    bf16 copy, like the bf16 forward, bitwise the f32 output rounded to nearest even."""
    g = sp.gen(n, 401)
    x, dy = torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g)
    k = min(n, len(SILU_FIXED))
    x[n - k:], dy[n - k:] = torch.tensor(SILU_FIXED[:k]), 1.0
    xd, dyd = _buf(n, fill=x), _buf(n, fill=dy)
    (rf, af), (rb, ab) = sp.silu_ref(x, dy)
    y, yb, dx, dx2, dxb = _buf(n), _buf(n, torch.bfloat16), _buf(n), _buf(n), _buf(n, torch.bfloat16)
    _ok(lib().vaw_silu_fwd(F32, ptr(xd), ptr(y), n, stream_ptr()))
    _ok(lib().vaw_silu_fwd(BF16, ptr(xd), ptr(yb), n, stream_ptr()))
    _ok(lib().vaw_silu_bwd(ptr(xd), ptr(dyd), ptr(dx), n, stream_ptr()))
    _ok(lib().vaw_silu_bwd_cast(ptr(xd), ptr(dyd), ptr(dx2), ptr(dxb), n, stream_ptr()))
    gy, gdx = _got(y, n), _got(dx, n)
    _check("vaw_silu_fwd", f"n={n}", gy, rf, af, False)
    _check("vaw_silu_bwd", f"n={n}", gdx, rb, ab, False)
    fx = slice(n - k, n)
    for name, got, ref in (("fwd", gy, rf), ("bwd", gdx, rb)):
        assert bool(torch.isfinite(got[fx]).all()), name
        assert torch.equal(torch.signbit(got[fx]), torch.signbit(ref[fx])), (name, got[fx].tolist(), ref[fx].tolist())
    assert float(gy[n - k]) == 0.0 and float(gdx[n - k]) == 0.5
    assert same_bits(_got(dx2, n), gdx) and same_bits(_got(dxb, n), sp.bf16_rne(gdx)) and same_bits(_got(yb, n), sp.bf16_rne(gy))
    for b, dt in ((y, 4), (yb, 2), (dx, 4), (dx2, 4), (dxb, 2)):
        assert _intact(b, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. vaw_add_embedding, vaw_embedding_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [(1, 1), (3, 260), (2100, 257)])
def test_add_embedding_and_its_nan_rule(B, D):
    """exact: one f32 addition per element -- the float64 sum rounded to f32, bit for bit; an index of -1 or `rows` gives a NaN row.
    2100 x 257 = 539700 elements: a second trip of the capped grid."""
    rows = 5
    g = sp.gen(B, D, 501)
    a, table = torch.randn(B, D, generator=g), torch.randn(rows, D, generator=g)
    idx = torch.randint(0, rows, (B,), generator=g)
    if B >= 3:
        idx[1], idx[B - 1] = -1, rows
    out, ad, tabd, idxd = _buf(B * D), a.to(DEV), table.to(DEV), idx.to(DEV)
    _ok(lib().vaw_add_embedding(ptr(ad), ptr(tabd), ptr(idxd), ptr(out), B, D, rows, stream_ptr()))
    got, ref = _got(out, B * D).view(B, D), sp.add_embedding_ref(a, table, idx)
    bad = (idx < 0) | (idx >= rows)
    assert bool(torch.isnan(got[bad]).all()) and same_bits(got[~bad], ref[~bad].float()) and _intact(out, B * D)


EMB_BWD = [(b, 5) for b in (1, 63, 64, 65, 1023, 1024, 1025, 2049)] + [(65, d) for d in (1, 255, 256, 257, 2048, 2049, 2304)]


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("B,D", EMB_BWD)
def test_embedding_bwd(B, D, beta):
    """B on the 64-entry mask and 1024-entry round edges, D below / on / above the 256 threads and on the second 2048-column trip.
    Index patterns: mixed (rows 0 .. 4 of 6 and, from B = 3 on, -1, rows and rows + 7, which are ignored) and every sample on row 2;
    row 5 is never hit: zero at beta = 0 (over a NaN-filled table), unchanged at beta = 1.
    exact: integers of [-2, 2], a column sums at most 2049 of them: below 4100.  random data: bitwise the f32 sum taken one row after
    the other in batch order on the CPU, the order the kernel promises."""
    rows = 6
    g = sp.gen(B, D, 601)
    mixed = torch.randint(0, rows - 1, (B,), generator=g)
    if B >= 3:
        mixed[0], mixed[B // 2], mixed[B - 1] = -1, rows, rows + 7
    for pattern, idx in (("mixed", mixed), ("same", torch.full((B,), 2))):
        for integer in (True, False):
            dc = sp.ints(g, B, D).float() if integer else torch.randn(B, D, generator=g)
            tab0 = (sp.ints(g, rows, D).float() if integer else torch.randn(rows, D, generator=g))
            tab, dcd, idxd = _buf(rows * D, fill=(tab0 if beta else NAN)), dc.to(DEV), idx.to(DEV)
            _ok(lib().vaw_embedding_bwd(ptr(dcd), ptr(idxd), ptr(tab), B, D, rows, beta, stream_ptr()))
            got = _got(tab, rows * D).view(rows, D)
            if integer:
                assert torch.equal(got.double(), sp.embedding_bwd_ref(dc.double(), idx, tab0.double(), beta)), (pattern, "integer")
            else:
                assert same_bits(got, sp.embedding_bwd_ref(dc, idx, tab0, beta)), (pattern, "random")
            assert same_bits(got[5], tab0[5] if beta else torch.zeros(D)), "the row nobody hits"
            assert _intact(tab, rows * D)


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. patch shuffles
# ------------------------------------------------------------------------------------------------------------------------------------
PATCH_GEOS = [(1, 1, 1, 1, 1), (2, 3, 6, 10, 2), (3, 4, 16, 24, 4), (1, 8, 8, 24, 8), (3, 4, 192, 232, 2)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geo", PATCH_GEOS, ids=lambda g: "x".join(map(str, g)))
def test_patch_shuffles(geo, dtype):
    """exact: every element is its own index (an arange, below 2^24; the bf16 token outputs are its nearest-even rounding), so any
    permutation error shows.  H != W, p = 1 and 534528 elements (a second trip of the capped grid) included."""
    B, C, H, W, p = geo
    n = B * C * H * W
    img = torch.arange(n, dtype=torch.float32).reshape(B, C, H, W)
    tokens = torch.arange(n, dtype=torch.float32).reshape(B, (H // p) * (W // p), C * p * p) + 0.5
    imgd, tokd = _buf(n, fill=img), _buf(n, fill=tokens)
    cast = (lambda q: q) if dtype == torch.float32 else sp.bf16_rne
    L, s = lib(), stream_ptr()
    tok = _buf(n, dtype)
    _ok(L.vaw_patchify(_dt(dtype), ptr(imgd), ptr(tok), B, C, H, W, p, s))
    assert same_bits(_got(tok, n).view_as(tokens), cast(sp.patchify_ref(img, p))) and _intact(tok, n)
    tok = _buf(n, dtype)
    _ok(L.vaw_unpatchify_bwd(_dt(dtype), ptr(imgd), ptr(tok), B, C, H, W, p, s))
    assert same_bits(_got(tok, n).view_as(tokens), cast(sp.unpatchify_bwd_ref(img, p))) and _intact(tok, n)
    if dtype == torch.float32:                                   # the two image-side entries read and write f32 only
        out = _buf(n)
        _ok(L.vaw_patchify_bwd(ptr(tokd), ptr(out), B, C, H, W, p, s))
        assert same_bits(_got(out, n).view_as(img), sp.patchify_bwd_ref(tokens, C, H, W, p)) and _intact(out, n)
        out = _buf(n)
        _ok(L.vaw_unpatchify(F32, ptr(tokd), ptr(out), B, C, H, W, p, s))
        assert same_bits(_got(out, n).view_as(img), sp.unpatchify_ref(tokens, C, H, W, p)) and _intact(out, n)
    assert same_bits(_got(imgd, n).view_as(img), img) and _intact(imgd, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. vaw_cast_colsum_bf16
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 252, 256, 260])
@pytest.mark.parametrize("M", [60, 61, 64, 65, 127, 129, 512])
def test_cast_colsum_unrolled_loop_edges_and_strides(M, N):
    """The unrolled loop runs while r + 60 < M and advances by 64 rows: M = 60 none of it for any row group, 61 for group 0 alone,
    64 for all four, 65 the remainder after it for group 0, 127 / 129 one and two trips with remainders, 512 eight trips.
    exact: integers of [-300, 300] (those above 256 round in bf16: the sums are of the stored values), a column sums to at most
    512 x 300 + 2 < 2^24; dst bitwise the nearest-even cast.  ld_src = N + 4, ld_dst = N + 8 with canaries in the padding columns."""
    lds, ldd = N + 4, N + 8
    g = sp.gen(M, N, 701)
    src, prev = sp.ints(g, M, N, lo=-300, hi=300).float(), sp.ints(g, N).float()
    for beta in (0.0, 1.0):
        s_host = torch.full((M, lds), sp.CANARY)
        s_host[:, :N] = src
        d_host = torch.full((M, ldd), sp.CANARY, dtype=torch.bfloat16)
        d_host[:, :N] = NAN
        sd, dd = _buf(M * lds, fill=s_host), _buf(M * ldd, torch.bfloat16, fill=d_host)
        cs = _buf(N, fill=(prev if beta else NAN))
        _ok(lib().vaw_cast_colsum_bf16(ptr(sd), lds, ptr(dd), ldd, M, N, ptr(cs), beta, stream_ptr()))
        want_dst, want_cs = sp.cast_colsum_ref(src, prev, beta)
        got = _got(dd, M * ldd).view(M, ldd)
        assert same_bits(got[:, :N].contiguous(), want_dst), f"beta={beta}"
        assert bool((got[:, N:] == sp.CANARY).all()) and _intact(dd, M * ldd), "dst padding columns"
        assert torch.equal(_got(cs, N).double(), want_cs) and _intact(cs, N), f"beta={beta}"
        assert same_bits(_got(sd, M * lds).view(M, lds), s_host) and _intact(sd, M * lds)


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. vaw_reduce_rows, vaw_reduce_rows_batched
# ------------------------------------------------------------------------------------------------------------------------------------
RED_R, RED_COLS = [1, 31, 32, 33, 1000], [1, 31, 32, 33, 100]


@pytest.mark.parametrize("N", RED_COLS)
@pytest.mark.parametrize("R", RED_R)
def test_reduce_rows(R, N):
    """32 interleaved row groups, 32 columns a block.  integer: exact (a column of at most 1000 values of [-2, 2] plus out).
    random: derived bound (ceil(R / 32) + 32 + 2) u (sum |partial| + |beta out|) (reduce_rows_ref)."""
    for integer in (True, False):
        part, prev = sp.reduce_case(R, N, integer)
        pd = _buf(R * N, fill=part)
        for beta in (0.0, 1.0):
            out = _buf(N, fill=(prev if beta else NAN))
            _ok(lib().vaw_reduce_rows(ptr(pd), R, N, ptr(out), beta, stream_ptr()))
            ref, allow = sp.reduce_rows_ref(part, prev, beta)
            _check("vaw_reduce_rows", f"{R}x{N} beta={beta}", _got(out, N), ref, allow, integer)
            assert _intact(out, N) and _intact(pd, R * N)


@pytest.mark.parametrize("integer", [True, False], ids=KINDS)
def test_reduce_rows_batched_mixed_jobs(integer):
    """all 25 shapes of test_reduce_rows as the jobs of one launch; the same comparison per job, and bitwise the unbatched fold"""
    shapes = [(R, N) for R in RED_R for N in RED_COLS]
    cases = [sp.reduce_case(R, N, integer, seed=3) for R, N in shapes]
    pds = [_buf(R * N, fill=c[0]) for (R, N), c in zip(shapes, cases)]
    for beta in (0.0, 1.0):
        outs = [_buf(N, fill=(c[1] if beta else NAN)) for (R, N), c in zip(shapes, cases)]
        grp = ops.ReduceGroup([(ptr(p), ptr(o), R, N) for (R, N), p, o in zip(shapes, pds, outs)], DEV)
        grp.launch(beta)
        torch.cuda.synchronize()
        for (R, N), c, p, o in zip(shapes, cases, pds, outs):
            ref, allow = sp.reduce_rows_ref(c[0], c[1], beta)
            ok = torch.equal(_got(o, N).double(), ref) if integer else within(_got(o, N), ref, allow)[0]
            assert ok and _intact(o, N), (R, N, beta)
            single = _buf(N, fill=(c[1] if beta else NAN))
            _ok(lib().vaw_reduce_rows(ptr(p), R, N, ptr(single), beta, stream_ptr()))
            assert same_bits(_got(single, N), _got(o, N)), (R, N, beta)


# ------------------------------------------------------------------------------------------------------------------------------------
# 10. base pointers one float past a 16-byte boundary with n % 4 == 0: the entries decide through vec4_ok and take the scalar loop
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_rows_match_the_reference_and_the_aligned_result(kind):
    """n = 1028 (a second block), every tensor one float off.  The elementwise entries (vaw_qsample_fwd, vaw_mix_rows, vaw_wmse_bwd,
    vaw_wmse_bwd_t) compute each element from the same operations on either path: bitwise the aligned result, and exact / inside the
    derived bound like it.  vaw_wmse_fwd / vaw_wmse_fwd_t add in another order on the scalar path: exact on the integer case, inside
    the derived bound of wmse_ref (which covers both paths' chains) on the random one."""
    B, n, integer = 3, 1028, kind == "integer"
    c = _mse_case(B, n, integer)
    t = c["t"].to(DEV)
    d0, d1 = _dev(c), _dev(c, off=1)
    assert _p(d1["x0"], 1) % 16 == 4
    ref, allow = sp.qsample_ref(c["x0"], c["noise"], c["t"], c["ca"], c["cb"])
    a, cc = c["ca"][c["t"]].to(DEV), c["cb"][c["t"]].to(DEV)
    for name, al, mis in (("vaw_qsample_fwd", _qsample(c, d0, t, B, n), _qsample(c, d1, t, B, n, off=1)),
                          ("vaw_mix_rows", _mix(c, d0, a, cc, B, n), _mix(c, d1, a, cc, B, n, off=1))):
        _check(name + " misaligned", kind, mis, ref, allow, integer)
        assert same_bits(al, mis), name
    for (name, al, _, _), (_, mis, ref, allow) in zip(_wmse_bwd_calls(c, d0, B, n, integer), _wmse_bwd_calls(c, d1, B, n, integer, off=1)):
        _check(name + " misaligned", kind, mis, ref, allow, integer)
        assert same_bits(al, mis), name
    tt = c["t"]
    ref, allow = sp.wmse_ref(c["out"], c["x0"], c["noise"], c["ca"][tt], c["cb"][tt], c["w"][tt])
    for name, got in _wmse_fwd_calls(c, d1, B, n, off=1):
        if integer:
            assert same_bits(got, _wmse_exact(c, n)), name
        else:
            _check(name + " misaligned", kind, got, ref, allow, False)
    for k in ("out", "x0", "noise"):
        assert _intact(d1[k], B * n, 1)

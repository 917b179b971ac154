"""The references and comparators of tests/step_parity.py, checked without a GPU: every reference against the oracle, every comparator
against a named wrong answer it must reject, and the allowance of every reduction case of test_gpu_step_kernels.py against its result
(below 1e-4 relative: a row whose terms cancelled to near zero would make a bound vacuous)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_parity as sp
from oracle import diffusion as od, dit as odit, unet as ounet

U = sp.U


# ------------------------------------------------------------------------------------------------------------------------------------
# references against the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
def _diffusion(mean_type, var_type, loss_type=od.LossType.MSE, weight_type="lambda"):
    args = SimpleNamespace(weight_type=weight_type, gamma=0.0, learn_sigma=False, p2_gamma=1, p2_k=1)
    return od.GaussianDiffusion(args=args, betas=od.get_named_beta_schedule("linear", sp.T_STEPS), model_mean_type=mean_type,
                                model_var_type=var_type, loss_type=loss_type)


@pytest.fixture
def wide_tables(monkeypatch):
    """the oracle gathers its tables as f32 and would go on in f32 wherever only tables meet (exp(logvar1 - logvar2) with a fixed
    variance): widen the gathered f32 values, so that it computes in float64 from the same table values the kernels are handed"""
    extract = od.extract
    monkeypatch.setattr(od, "extract", lambda arr, t, shape: extract(arr, t, shape).double())


VB_ORACLE = [  # mean_mode, var_mode, table kind, oracle types
    (0, 0, "large", od.ModelMeanType.EPSILON, od.ModelVarType.FIXED_LARGE),
    (0, 0, "small", od.ModelMeanType.EPSILON, od.ModelVarType.FIXED_SMALL),
    (0, 1, "learned", od.ModelMeanType.EPSILON, od.ModelVarType.LEARNED),
    (0, 2, "learned", od.ModelMeanType.EPSILON, od.ModelVarType.LEARNED_RANGE),
    (1, 0, "large", od.ModelMeanType.PREVIOUS_X, od.ModelVarType.FIXED_LARGE),
    (1, 1, "learned", od.ModelMeanType.PREVIOUS_X, od.ModelVarType.LEARNED),
    (1, 2, "learned", od.ModelMeanType.PREVIOUS_X, od.ModelVarType.LEARNED_RANGE),
]


@pytest.mark.parametrize("mean_mode,var_mode,kind,mt,vt", VB_ORACLE, ids=lambda v: str(getattr(v, "name", v)))
def test_vb_restatement_matches_the_oracle_in_float64(wide_tables, mean_mode, var_mode, kind, mt, vt):
    """vb_ref (p_mean_variance + vb_elem on table rows) against _vb_terms_bpd, and its pieces against normal_kl and
    discretized_gaussian_log_likelihood, all on float64 tensors; the analytic gradients of vb_elem against autograd."""
    d = _diffusion(mt, vt)
    c = sp.vb_case(75, mean_mode, var_mode, seed=3)
    t = torch.tensor(sp.VB_T)
    C, H = 3, 5
    sh = lambda q: q.double().reshape(3, C, H, H)
    model_out = sh(c["mean_out"]) if var_mode == 0 else torch.cat([sh(c["mean_out"]), sh(c["var_out"])], 1)
    coef = sp.table_rows(d, mean_mode, kind)[t]
    want = d._vb_terms_bpd(model_out, sh(c["x0"]), sh(c["xt"]), t)
    got = sp.vb_ref(c["mean_out"], c["var_out"], c["x0"], c["xt"], coef, mean_mode, var_mode, 1.0)
    assert want.dtype == torch.float64
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
    # the pieces, elementwise
    m, v, x, z = (None if q is None else q.double() for q in (c["mean_out"], c["var_out"], c["x0"], c["xt"]))
    cols = sp._vb_cols(coef, torch.float64)
    mean, lv = sp.p_mean_variance(cols, mean_mode, var_mode, m, v, z)
    lv = lv.expand_as(x)
    tm, tlv = cols[2] * x + cols[3] * z, cols[4].expand_as(x)
    val, dlv, dmean = sp.vb_elem(x, tm, tlv, mean, lv, coef[:, 11:12] != 0)
    torch.testing.assert_close(val[1:], od.normal_kl(tm, tlv, mean, lv)[1:], rtol=1e-12, atol=1e-15)
    nll = -od.discretized_gaussian_log_likelihood(x, means=mean, log_scales=0.5 * lv)
    torch.testing.assert_close(val[:1], nll[:1], rtol=1e-12, atol=1e-15)
    assert bool((val[0, c["floors"]] == -np.log(1e-12)).all()), "the floor elements must sit on the floor"
    # analytic gradients (what the kernel computes) against autograd of the value
    mean_r, lv_r = mean.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    sp.vb_elem(x, tm, tlv, mean_r, lv_r, coef[:, 11:12] != 0)[0].sum().backward()
    torch.testing.assert_close(dmean, mean_r.grad, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(dlv, lv_r.grad, rtol=1e-9, atol=1e-12)
    assert bool((dmean[0, c["floors"]] == 0).all()) and bool((dlv[0, c["floors"]] == 0).all())


def test_qsample_and_weighted_mse_match_the_oracle(wide_tables):
    """q_sample and training_losses["mse"] (VELOCITY target: both coefficients live; weight alpha * sigma) on float64 tensors, and
    the gradient of sum_b gm[b] mse[b] by autograd through the oracle"""
    d = _diffusion(od.ModelMeanType.VELOCITY, od.ModelVarType.FIXED_LARGE)
    B, C, H = 4, 3, 5
    g = sp.gen(B, C, H)
    x0, noise, out = (torch.randn(B, C, H, H, generator=g).double() for _ in range(3))
    t = torch.tensor([0, 999, 17, 640])
    f = lambda arr: torch.from_numpy(arr).float()
    tab_a, tab_s = f(d.sqrt_alphas_cumprod), f(d.sqrt_one_minus_alphas_cumprod)
    xt, _ = sp.qsample_ref(x0.reshape(B, -1), noise.reshape(B, -1), t, tab_a, tab_s)
    torch.testing.assert_close(xt.reshape(B, C, H, H), d.q_sample(x0, t, noise=noise), rtol=1e-14, atol=0)
    o = out.clone().requires_grad_(True)
    terms = d.training_losses(lambda x, tt, **kw: o, x0, t=t, noise=noise)
    # target = alpha noise - sigma x0: ca = -sigma, cb = alpha, w = alpha * sigma
    a, s = tab_a[t], tab_s[t]
    mse, _ = sp.wmse_ref(out.reshape(B, -1), x0.reshape(B, -1), noise.reshape(B, -1), -s, a, a.double() * s.double())
    torch.testing.assert_close(mse, terms["mse"].detach().double(), rtol=1e-13, atol=0)
    gm = torch.rand(B, generator=g).double() + 0.5
    (terms["mse"] * gm).sum().backward()
    grad, _ = sp.wmse_grad_ref(out.reshape(B, -1), x0.reshape(B, -1), noise.reshape(B, -1), -s, a, a.double() * s.double(), gm)
    torch.testing.assert_close(grad.reshape(B, C, H, H), o.grad, rtol=1e-12, atol=1e-18)
    mean, _ = sp.batch_mean_ref(mse.float(), 2.0)
    torch.testing.assert_close(mean, mse.float().double().mean() / 2.0, rtol=1e-15, atol=0)


def test_latent_qsample_is_the_sample_then_the_mix():
    B, n = 3, 12
    g = sp.gen(B, n, 7)
    latent, eps, noise = torch.randn(B, 2, n, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    tab_a, tab_s = torch.rand(sp.T_STEPS, generator=g), torch.rand(sp.T_STEPS, generator=g)
    t = torch.tensor([0, 999, 5])
    x0, _, xt, _, tf = sp.latent_qsample_ref(latent, eps, noise, t, tab_a, tab_s, 0.18215, 0.25)
    want = (latent[:, 0].double() + latent[:, 1].double() * eps.double()) * float(np.float32(0.18215))
    torch.testing.assert_close(x0, want, rtol=1e-15, atol=0)
    torch.testing.assert_close(xt, sp.mix_ref(x0, noise, tab_a[t], tab_s[t])[0], rtol=1e-15, atol=0)
    assert tf.tolist() == [0.0, 249.75, 1.25]


@pytest.mark.parametrize("dim", [1, 2, 33, 64, 257])
def test_sinusoidal_embedding_matches_the_oracle(dim):
    """the oracle evaluates in f32: it must sit inside the allowance around the float64 reference, and the odd column is zero"""
    t = torch.tensor([0.0, 0.5, 999.0, 123.25])
    ref, allow = sp.timestep_embedding_ref(t, dim)
    if dim == 1:             # no frequency at all: the oracle's zeros_like(emb[:, :1]) of an empty tensor is empty; the kernel's column is zero
        assert ref.shape == (4, 1) and bool((ref == 0).all()) and bool((allow == 0).all())
        return
    want = ounet.timestep_embedding(t, dim)
    assert want.shape == ref.shape
    ok, ratio = sp.within(want, ref, allow)
    assert ok, ratio
    if dim % 2:
        assert bool((ref[:, -1] == 0).all()) and bool((allow[:, -1] == 0).all())
    if dim >= 2:
        assert bool((ref[0, :dim // 2] == 1).all()) and bool((ref[0, dim // 2:] == 0).all())       # t = 0: cos 1, sin 0
        assert float((allow / ref.abs().clamp_min(1.0)).max()) < 1e-2


def test_silu_reference_matches_torch_and_its_derivative():
    x = torch.cat([torch.randn(1000, generator=sp.gen(5)) * 3, torch.tensor([0.0, 1e-6, -1e-6, 20.0, -20.0, 87.0, -87.0])])
    dy = torch.randn(x.numel(), generator=sp.gen(6))
    (f, fa), (b, ba) = sp.silu_ref(x, dy)
    xr = x.double().requires_grad_(True)
    y = F.silu(xr)
    (y * dy.double()).sum().backward()
    torch.testing.assert_close(f, y.detach(), rtol=1e-13, atol=1e-300)
    torch.testing.assert_close(b, xr.grad, rtol=1e-12, atol=1e-300)
    ok, _ = sp.within(F.silu(x), f, fa)          # torch's f32 SiLU sits inside the allowance
    assert ok
    assert float((fa / f.abs().clamp_min(1e-30))[x.abs() <= 20].max()) < 1e-5 and bool(torch.isfinite(fa).all() and torch.isfinite(ba).all())


SHUFFLE_GEOS = [(1, 1, 1, 1, 1), (2, 3, 6, 10, 2), (3, 4, 16, 24, 4), (1, 8, 8, 24, 8)]


@pytest.mark.parametrize("geo", SHUFFLE_GEOS, ids=lambda g: "x".join(map(str, g)))
def test_patch_shuffles_match_the_index_formulas_and_the_oracle(geo):
    B, C, H, W, p = geo
    img = torch.arange(B * C * H * W, dtype=torch.float64).reshape(B, C, H, W)
    hp, wp = H // p, W // p
    tok, tok2 = sp.patchify_ref(img, p), sp.unpatchify_bwd_ref(img, p)
    for b, c, y, x in [(B - 1, C - 1, H - 1, W - 1), (0, 0, 0, 0), (B // 2, C // 2, H // 2, (W * 2) // 3)]:
        row, i, j = (y // p) * wp + x // p, y % p, x % p
        assert tok[b, row, (c * p + i) * p + j] == img[b, c, y, x]           # Conv2d weight order
        assert tok2[b, row, (i * p + j) * C + c] == img[b, c, y, x]          # final-layer order
    assert torch.equal(sp.patchify_bwd_ref(tok, C, H, W, p), img) and torch.equal(sp.unpatchify_ref(tok2, C, H, W, p), img)
    # patchify is the operand of the patch-embedding convolution
    w = torch.randn(5, C, p, p, generator=sp.gen(*geo)).double()
    torch.testing.assert_close(tok @ w.reshape(5, -1).T, F.conv2d(img, w, stride=p).flatten(2).transpose(1, 2), rtol=1e-12, atol=1e-9)
    if H == W:                                                                # the oracle's unpatchify is square only
        ns = SimpleNamespace(out_channels=C, x_embedder=SimpleNamespace(patch_size=(p, p)))
        assert torch.equal(odit.DiT.unpatchify(ns, tok2), img)


def test_square_unpatchify_matches_the_oracle():
    B, C, H, p = 2, 4, 8, 2
    tok = torch.randn(B, (H // p) ** 2, p * p * C, generator=sp.gen(1)).double()
    ns = SimpleNamespace(out_channels=C, x_embedder=SimpleNamespace(patch_size=(p, p)))
    img = odit.DiT.unpatchify(ns, tok)
    assert torch.equal(sp.unpatchify_ref(tok, C, H, H, p), img) and torch.equal(sp.unpatchify_bwd_ref(img, p), tok)


def test_embedding_references_match_torch():
    g = sp.gen(11)
    rows, B, D = 7, 40, 5
    table, a = torch.randn(rows, D, generator=g), torch.randn(B, D, generator=g)
    idx = torch.randint(0, rows, (B,), generator=g)
    idx[3], idx[9] = -1, rows
    out = sp.add_embedding_ref(a, table, idx)
    ok = (idx >= 0) & (idx < rows)
    torch.testing.assert_close(out[ok], a.double()[ok] + F.embedding(idx[ok], table.double()), rtol=0, atol=0)
    assert bool(torch.isnan(out[~ok]).all())
    dc = sp.ints(g, B, D)
    tab0 = sp.ints(g, rows, D)
    w = torch.zeros(rows, D, dtype=torch.float64, requires_grad=True)
    (F.embedding(idx[ok], w) * dc[ok]).sum().backward()
    assert torch.equal(sp.embedding_bwd_ref(dc, idx, tab0, 0.0), w.grad)
    assert torch.equal(sp.embedding_bwd_ref(dc, idx, tab0, 1.0), tab0 + w.grad)


def test_cast_colsum_and_reduce_rows_references():
    g = sp.gen(13)
    src = sp.ints(g, 61, 8, lo=-300, hi=300).float()
    prev = sp.ints(g, 8).float()
    dst, cs = sp.cast_colsum_ref(src, prev, 1.0)
    assert torch.equal(dst, src.bfloat16()) and torch.equal(cs, prev.double() + src.bfloat16().double().sum(0))
    assert not torch.equal(cs, prev.double() + src.double().sum(0)), "the sums are of the stored values: 257 must have rounded"
    part, out = sp.reduce_case(33, 5, True)
    val, _ = sp.reduce_rows_ref(part, out, 1.0)
    assert torch.equal(val, out.double() + part.double().sum(0))


# ------------------------------------------------------------------------------------------------------------------------------------
# each comparator rejects its named wrong answer
# ------------------------------------------------------------------------------------------------------------------------------------
def test_exact_comparator_rejects_swapped_token_order():
    """(c, i, j) against (i, j, c)"""
    img = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6)
    assert sp.patchify_ref(img, 2).shape == sp.unpatchify_bwd_ref(img, 2).shape
    assert not torch.equal(sp.patchify_ref(img, 2), sp.unpatchify_bwd_ref(img, 2))
    tok = sp.patchify_ref(img, 2)
    assert not torch.equal(sp.patchify_bwd_ref(tok, 3, 4, 6, 2), sp.unpatchify_ref(tok, 3, 4, 6, 2))


@pytest.mark.parametrize("n", [1 + 1, 75, 4096, 4100, 12292])
def test_bounds_reject_a_reduction_without_its_last_element(n):
    c = sp.mse_case(3, n, False)
    t = sp.timesteps(3)
    a, cc, w = c["ca"][t], c["cb"][t], c["w"][t]
    ref, allow = sp.wmse_ref(c["out"], c["x0"], c["noise"], a, cc, w)
    assert float((allow / ref.abs()).max()) < 1e-4
    short, _ = sp.wmse_ref(c["out"][:, :-1], c["x0"][:, :-1], c["noise"][:, :-1], a, cc, w)
    wrong = short * (n - 1) / n                                  # the same sum of squares without the last term, over n
    assert sp.within(ref.float(), ref, allow)[0] and not sp.within(wrong, ref, allow)[0]
    assert not sp.within(wrong.float(), ref, allow)[0]


@pytest.mark.parametrize("B", [2, 255, 256, 257, 700])
def test_batch_mean_bound_rejects_a_missing_last_row(B):
    v = torch.rand(B, generator=sp.gen(B, 17)) + 0.5
    ref, allow = sp.batch_mean_ref(v, 2.0)
    assert float(allow / ref) < 1e-4
    assert sp.within(v.sum() / B / 2.0, ref, allow)[0]
    assert not sp.within(v[:-1].double().sum() / B / 2.0, ref, allow)[0]


@pytest.mark.parametrize("R,N", [(2, 1), (31, 31), (32, 32), (33, 33), (1000, 100)])
def test_reduce_rows_bound_rejects_a_missing_row_and_ignored_beta(R, N):
    part, out = sp.reduce_case(R, N, False)
    for beta in (0.0, 1.0):
        ref, allow = sp.reduce_rows_ref(part, out, beta)
        assert float((allow / ref.abs()).max()) < 1e-4
        good = (part.sum(0) + beta * out)
        assert sp.within(good, ref, allow)[0]
        assert not sp.within(part[:-1].sum(0) + beta * out, ref, allow)[0], "last row left out"
    ref, allow = sp.reduce_rows_ref(part, out, 1.0)
    assert not sp.within(part.sum(0), ref, allow)[0], "beta ignored"
    # and on the integer cases the comparison is exact
    part, out = sp.reduce_case(R, N, True)
    assert not torch.equal(sp.reduce_rows_ref(part, out, 1.0)[0], sp.reduce_rows_ref(part, out, 0.0)[0])


def test_bounds_reject_a_coefficient_gathered_at_t_plus_one():
    d = sp.oracle_diffusion()
    f = lambda arr: torch.from_numpy(arr).float()
    tab_a, tab_s = f(d.sqrt_alphas_cumprod), f(d.sqrt_one_minus_alphas_cumprod)
    c = sp.mse_case(3, 75, False)
    t = torch.tensor([0, 500, 998])
    ref, allow = sp.qsample_ref(c["x0"], c["noise"], t, tab_a, tab_s)
    assert sp.within((tab_a[t][:, None] * c["x0"] + tab_s[t][:, None] * c["noise"]), ref, allow)[0]
    wrong, _ = sp.qsample_ref(c["x0"], c["noise"], t + 1, tab_a, tab_s)
    for b in range(3):
        assert not sp.within(wrong[b], ref[b], allow[b])[0], f"row {b}"
    # the weighted MSE and its gradient gather the same way
    mse, ma = sp.wmse_ref(c["out"], c["x0"], c["noise"], tab_a[t], tab_s[t], tab_s[t])
    wrong, _ = sp.wmse_ref(c["out"], c["x0"], c["noise"], tab_a[t + 1], tab_s[t + 1], tab_s[t + 1])
    assert not sp.within(wrong, mse, ma)[0]
    # out-of-range timesteps poison the row
    bad, _ = sp.qsample_ref(c["x0"], c["noise"], torch.tensor([-1, 1000, 5]), tab_a, tab_s)
    assert bool(torch.isnan(bad[:2]).all()) and bool(torch.isfinite(bad[2]).all())


@pytest.mark.parametrize("n,mean_mode,var_mode", [(n, mm, vm) for n in (75, 4100) for mm, vm in sp.VB_MODES] + [(n, 0, 2) for n in (1, 4096, 12292)])
def test_vb_allowance_is_small_and_rejects_the_wrong_bin_and_a_missing_element(n, mean_mode, var_mode):
    c = sp.vb_case(n, mean_mode, var_mode)
    args = (c["mean_out"], c["var_out"], c["x0"], c["xt"], c["coef"], mean_mode, var_mode, c["scale"])
    ref = sp.vb_ref(*args)
    allow, mag = sp.vb_fwd_allow(*args)
    assert bool(torch.isfinite(allow).all()) and float((allow / ref.abs()).max()) < 1e-4
    assert bool((mag * c["scale"] / (n * sp.LN2) < 4 * ref.abs()).all()), "a row's value must not be a cancelled remainder"
    if n == 1:               # one element a row (row 0: on its floor under either formula): nothing to leave out
        return
    wrong = sp.vb_ref(*args, wrong_open_bins=True)               # the middle bin's formula in the open-ended bins
    assert not sp.within(wrong[:1], ref[:1], allow[:1])[0] and torch.equal(wrong[1:], ref[1:])
    cut = lambda q: None if q is None else q[:, :-1]
    short = sp.vb_ref(cut(c["mean_out"]), cut(c["var_out"]), cut(c["x0"]), cut(c["xt"]), c["coef"], mean_mode, var_mode, c["scale"])
    for b in range(3):
        assert not sp.within(short[b] * (n - 1) / n, ref[b], allow[b])[0], f"row {b}: last element left out"
    for r, a in sp.vb_bwd_allow(*args, c["gvb"]):
        if r is not None:
            assert bool(torch.isfinite(a).all()) and float((a.amax(1) / r.abs().amax(1)).max()) < 1e-3
            assert bool((r[0, c["floors"]] == 0).all()) and bool((a[0, c["floors"]] == 0).all()), "zero gradient on the floors, exactly"


def test_embedding_scatter_rejects_reverse_order_and_ignored_beta():
    g = sp.gen(19)
    B, D, rows = 65, 257, 4
    dc, idx = torch.randn(B, D, generator=g), torch.randint(0, rows - 1, (B,), generator=g)
    tab = torch.randn(rows, D, generator=g)
    fwd, rev = sp.embedding_bwd_ref(dc, idx, tab, 1.0), sp.embedding_bwd_ref(dc, idx, tab, 1.0, reverse=True)
    assert fwd.dtype == torch.float32 and not sp.same_bits(fwd, rev), "a sum in reverse batch order must differ in some bit"
    assert not sp.same_bits(fwd, sp.embedding_bwd_ref(dc, idx, tab, 0.0))
    assert sp.same_bits(fwd[rows - 1], tab[rows - 1]) and bool((sp.embedding_bwd_ref(dc, idx, tab, 0.0)[rows - 1] == 0).all())
    torch.testing.assert_close(fwd.double(), sp.embedding_bwd_ref(dc.double(), idx, tab, 1.0), rtol=1e-5, atol=1e-5)


def test_bf16_comparator_rejects_truncation():
    x = torch.randn(4096, generator=sp.gen(23))
    trunc = (x.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert not sp.same_bits(trunc, sp.bf16_rne(x))
    assert sp.same_bits(sp.bf16_rne(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])), torch.tensor([1.0, 1.0 + 2.0 ** -6]).bfloat16())
    src = sp.ints(sp.gen(29), 64, 4, lo=-300, hi=300).float()
    dst, cs = sp.cast_colsum_ref(src, torch.zeros(4), 0.0)
    tr = (src.view(torch.int32) & -65536).view(torch.float32)
    assert not torch.equal(cs, tr.double().sum(0)) and not sp.same_bits(dst, tr.bfloat16())


def test_silu_allowance_rejects_a_one_percent_error_and_the_sigmoid_alone():
    x = torch.randn(257, generator=sp.gen(31)) * 3
    dy = torch.randn(257, generator=sp.gen(37))
    (f, fa), (b, ba) = sp.silu_ref(x, dy)
    assert not sp.within(f * (1 + 1e-5), f, fa)[0]
    assert not sp.within(dy.double() * torch.sigmoid(x.double()), b, ba)[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# the exact integer cases stay below 2^24
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 75, 4096, 4100, 12292, 65543])
def test_integer_mse_case_is_exact_in_f32(n):
    c = sp.mse_case(3, n, True)
    t = sp.timesteps(3)
    a, cc = c["ca"][t].double()[:, None], c["cb"][t].double()[:, None]
    d = a * c["x0"].double() + cc * c["noise"].double() - c["out"].double()
    assert float(d.abs().max()) <= 10 and bool((d * 2 == (d * 2).round()).all())
    assert float((d * d).sum(1).max()) * 4 < 2 ** 24
    xt, _ = sp.mix_ref(c["x0"], c["noise"], c["ca"][t], c["cb"][t])
    assert torch.equal(xt.float().double(), xt)

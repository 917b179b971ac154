"""Host side of likelihood evaluation (calc_bpd_loop, DDIM inversion) without a GPU: the table methods on CPU tensors
against what the unmodified reference produced (tests/golden/eval_bpd.pt), and the bookkeeping of the loop -- column
order, noise order, t_chunk stacking, SpacedDiffusion wrapping -- with a recording model and torch stand-ins for the three
kernel wrappers the loop calls."""
import math

import numpy as np
import pytest
import torch

from conftest import base_args, load_pt

import vaw_amd
from vaw_amd import gaussian_diffusion as vgd

# name -> schedule, base T, mean type, var type, respacing (None = plain GaussianDiffusion), rescale_timesteps, clip_denoised
# (the settings tests/golden/make_eval_goldens.py ran the reference with)
BPD_CASES = {
    "lin_eps_range_50": ("linear", 1000, "EPSILON", "LEARNED_RANGE", "50", True, True),
    "cos_x0_large_20": ("cosine", 1000, "START_X", "FIXED_LARGE", "20", True, True),
    "lin_xprev_small_25": ("linear", 1000, "PREVIOUS_X", "FIXED_SMALL", "25", True, True),
    "lin_eps_range_1000": ("linear", 1000, "EPSILON", "LEARNED_RANGE", "1000", True, True),
    "lin_x0_learned_15_noclip": ("linear", 1000, "START_X", "LEARNED", "15", True, False),
    "plain_lin_x0_small_100": ("linear", 100, "START_X", "FIXED_SMALL", None, False, True),
}


def make_diffusion(sched, T, mt, vt, respacing, rescale, **args_kw):
    # 'lambda' has no PREVIOUS_X weight (training side); evaluation does not use the weight
    wt = "constant" if mt == "PREVIOUS_X" else "lambda"
    kw = dict(args=base_args(weight_type=wt, learn_sigma=vt.startswith("LEARNED"), **args_kw),
              betas=vaw_amd.get_named_beta_schedule(sched, T), model_mean_type=vaw_amd.ModelMeanType[mt],
              model_var_type=vaw_amd.ModelVarType[vt], loss_type=vaw_amd.LossType.MSE, rescale_timesteps=rescale)
    if respacing is None:
        return vaw_amd.GaussianDiffusion(**kw)
    return vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(T, respacing), **kw)


@pytest.mark.parametrize("name", list(BPD_CASES))
def test_q_methods_on_cpu_vs_reference(name):
    g = load_pt("eval_bpd.pt")
    rec, x0 = g["bpd"][name], g["x0"]
    d = make_diffusion(*BPD_CASES[name][:6])
    assert d.num_timesteps == rec["n"]
    for i, t in enumerate(rec["q_t"]):
        x_t = rec["q_x_t"][i]
        for got, exp in zip(d.q_mean_variance(x0, t), rec["q_mean_variance"][i]):
            assert got.shape == x0.shape
            torch.testing.assert_close(got, exp, rtol=1e-6, atol=0)
        for got, exp in zip(d.q_posterior_mean_variance(x0, x_t, t), rec["q_posterior_mean_variance"][i]):
            assert got.shape == x0.shape
            torch.testing.assert_close(got, exp, rtol=1e-6, atol=1e-7 * float(exp.abs().max()))
        exp = rec["eps_from_xstart"][i]
        torch.testing.assert_close(d._predict_eps_from_xstart(x_t, t, x0), exp, rtol=1e-6, atol=1e-7 * float(exp.abs().max()))


@pytest.mark.parametrize("name", list(BPD_CASES))
def test_prior_bpd_table_scalars_vs_reference(name):
    """The two f32 scalars vaw_prior_bpd receives, put through the kernel's formula in torch, give the reference's
    _prior_bpd; and they are the f32 casts of the float64 tables at T-1."""
    g = load_pt("eval_bpd.pt")
    rec, x0 = g["bpd"][name], g["x0"]
    d = make_diffusion(*BPD_CASES[name][:6])
    a, lv = d._prior_coefs()
    assert a == float(np.float32(np.sqrt(d.alphas_cumprod[-1]))) and lv == float(np.float32(np.log(1.0 - d.alphas_cumprod[-1])))
    a, lv = torch.tensor(a), torch.tensor(lv)
    kl = 0.5 * (-1.0 - lv + torch.exp(lv) + (a * x0) ** 2)
    got = kl.mean(dim=(1, 2, 3)) / math.log(2.0)
    torch.testing.assert_close(got, rec["prior_bpd"], rtol=1e-5, atol=0)
    assert torch.equal(rec["prior_bpd"], rec["prior_only"])


def test_sample_table_carries_alphas_cumprod_next_in_a_spare_column():
    d = make_diffusion("linear", 1000, "EPSILON", "LEARNED_RANGE", "50", True)
    tab = d._sample_table()
    assert tab.shape == (50, 16) and tab.dtype == torch.float32
    assert torch.equal(tab[:, 13], torch.from_numpy(d.alphas_cumprod_next).float())
    assert torch.equal(tab[:, 14:], torch.zeros(50, 2))
    assert torch.equal(tab[:, 10], torch.from_numpy(d.alphas_cumprod_prev).float()) and tab[0, 11] == 1 and tab[1:, 11].abs().sum() == 0


# ---- the loop's bookkeeping -------------------------------------------------------------------------------------------
class FakeOps:
    """torch stand-ins for the three wrappers calc_bpd_loop calls (the real ones refuse CPU tensors); each records its call."""

    def __init__(self):
        self.calls = []

    def qsample(self, x0, noise, t, tab_a, tab_s):
        return tab_a[t].view(-1, 1, 1, 1) * x0 + tab_s[t].view(-1, 1, 1, 1) * noise

    def bpd_terms(self, mean_out, var_out, x0, x_t, noise, coef, mean_mode, var_mode, clip_denoised, out=None, col=0, group=None):
        B = x0.shape[0]
        self.calls.append(dict(B=B, col=col, group=group, noise=noise.clone(), coef=coef.clone(), x0=x0.clone(), clip=clip_denoised,
                               modes=(mean_mode, var_mode), has_var=var_out is not None))
        b = torch.arange(B)
        vals = (mean_out.flatten(1).mean(1), (x_t - x0).flatten(1).pow(2).mean(1), noise.flatten(1).pow(2).mean(1))
        for o, v in zip(out, vals):
            o[b % group, col + b // group] = v
        return out

    def prior_bpd(self, x0, a, lv):
        return torch.full((x0.shape[0],), 0.25)


class Recorder:
    def __init__(self, channels_out):
        self.seen = []
        self.mult = channels_out

    def __call__(self, x, t, **kw):
        self.seen.append((x.shape[0], t.clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}))
        m = 0.5 * x + 1e-3 * t.view(-1, 1, 1, 1).float() + 0.01 * kw["y"].view(-1, 1, 1, 1).float()
        return torch.cat([m] * self.mult, dim=1)


def run_loop(monkeypatch, d, K, cpu_rng, learned=True, **kw):
    fake = FakeOps()
    monkeypatch.setattr(vgd, "ops", fake)
    d.args.cpu_rng = cpu_rng
    model = Recorder(2 if learned else 1)
    x0 = torch.randn(3, 2, 4, 4, generator=torch.Generator().manual_seed(1)).clamp(-1, 1)
    torch.manual_seed(77)
    out = d.calc_bpd_loop(model, x0, model_kwargs={"y": torch.tensor([4, 2, 7]), "flag": "keep"}, t_chunk=K, **kw)
    return out, model, fake, torch.get_rng_state(), x0


@pytest.mark.parametrize("cpu_rng", [True, False])
def test_loop_column_order_noise_order_and_t_chunk_stacking(monkeypatch, cpu_rng):
    T = 10
    d = make_diffusion("cosine", T, "EPSILON", "LEARNED_RANGE", None, False)
    ref, model1, fake1, state1, x0 = run_loop(monkeypatch, d, 1, cpu_rng)
    assert set(ref) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"}
    assert ref["vb"].shape == ref["mse"].shape == ref["xstart_mse"].shape == (3, T) and ref["total_bpd"].shape == (3,)
    torch.testing.assert_close(ref["total_bpd"], ref["vb"].sum(dim=1) + ref["prior_bpd"])
    # the reference's loop: t = T-1 .. 0, one model call and one draw per timestep, column j = timestep T-1-j
    assert [int(t[0]) for _, t, _ in model1.seen] == list(range(T - 1, -1, -1))
    torch.manual_seed(77)
    draws = [torch.randn(3, 2, 4, 4) for _ in range(T)]
    assert torch.equal(torch.get_rng_state(), state1)
    tab = d._sample_table()
    for j, c in enumerate(fake1.calls):
        assert c["B"] == 3 and c["col"] == j and c["group"] == 3 and c["clip"] is True and c["modes"] == (0, 2) and c["has_var"]
        assert torch.equal(c["noise"], draws[j]) and torch.equal(c["coef"], tab[T - 1 - j].expand(3, 16))
        torch.testing.assert_close(ref["mse"][:, j], draws[j].flatten(1).pow(2).mean(1))
    for K in (4, 7, T, 3 * T):
        out, model, fake, state, _ = run_loop(monkeypatch, d, K, cpu_rng)
        k_eff = min(K, T)
        sizes = [k_eff] * (T // k_eff) + ([T % k_eff] if T % k_eff else [])
        assert [c["B"] for c in fake.calls] == [3 * s for s in sizes] and [n for n, _, _ in model.seen] == [3 * s for s in sizes]
        assert [c["col"] for c in fake.calls] == [sum(sizes[:i]) for i in range(len(sizes))]
        j = 0
        for (n, t, kw), c, s in zip(model.seen, fake.calls, sizes):
            # rows are timestep-major: [t_j]*N, [t_j - 1]*N, ...; per-sample kwargs repeat with them, others pass through
            assert t.tolist() == [T - 1 - (j + i) for i in range(s) for _ in range(3)]
            assert kw["y"].tolist() == [4, 2, 7] * s and kw["flag"] == "keep"
            assert torch.equal(c["noise"], torch.cat(draws[j:j + s])) and torch.equal(c["x0"], x0.repeat(s, 1, 1, 1))
            j += s
        assert torch.equal(state, state1), f"t_chunk={K} leaves another RNG state"
        for k in ref:
            assert torch.equal(out[k], ref[k]), f"t_chunk={K}: {k}"
    with pytest.raises(ValueError):
        run_loop(monkeypatch, d, 0, cpu_rng)


def test_loop_under_spaced_diffusion_sees_original_rescaled_timesteps(monkeypatch):
    d = make_diffusion("linear", 1000, "START_X", "FIXED_SMALL", "10", True)
    out, model, fake, _, _ = run_loop(monkeypatch, d, 4, True, learned=False, clip_denoised=False)
    kept = sorted(vaw_amd.space_timesteps(1000, "10"))
    assert d.timestep_map == kept
    seen = torch.cat([t for _, t, _ in model.seen])
    assert seen.dtype == torch.float32                         # rescale_timesteps: k * 1000 / T_original as float
    assert seen.tolist() == [float(kept[j]) for j in range(9, -1, -1) for _ in range(3)]
    assert all(c["clip"] is False and c["modes"] == (0, 0) and not c["has_var"] for c in fake.calls)
    assert out["vb"].shape == (3, 10)


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------
def test_refusals():
    x = torch.zeros(2, 3, 4, 4)
    t = torch.zeros(2, dtype=torch.long)
    model = lambda x, t, **kw: x
    d = make_diffusion("linear", 100, "EPSILON", "FIXED_SMALL", None, False)
    with pytest.raises(AssertionError):
        d.ddim_reverse_sample(model, x, t, eta=0.5)
    with pytest.raises(NotImplementedError):
        d.ddim_reverse_sample(model, x, t, denoised_fn=lambda v: v)
    v = make_diffusion("linear", 100, "VELOCITY", "FIXED_SMALL", None, False)
    with pytest.raises(RuntimeError, match="VELOCITY"):
        v.calc_bpd_loop(model, x)
    with pytest.raises(RuntimeError, match="VELOCITY"):
        v.ddim_reverse_sample(model, x, t)
    # the kernel wrappers have no CPU path
    coef = torch.zeros(2, 16)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.bpd_terms(x, None, x, x, x, coef, 0, 0, True)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.prior_bpd(x, 0.1, -0.1)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.ddim_reverse_step(x, x, coef, True)
    with pytest.raises(vaw_amd.VawError):
        d._prior_bpd(x)
    with pytest.raises(vaw_amd.VawError):
        d.calc_bpd_loop(model, x)


def test_new_entry_points_are_bound():
    lib = vaw_amd.lib()
    for name in ("vaw_bpd_terms", "vaw_prior_bpd", "vaw_guided_sample_step"):
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """per_sample <= 0, null required pointers, unknown modes and an impossible output layout come back as VAW_ERR_INVALID
    with a message in vaw_last_error_string; nothing is launched (the non-null addresses below are never dereferenced)."""
    lib = vaw_amd.lib()
    P = 4096                                                # a non-null placeholder address

    def bpd(mean=P, var=P, ld=64, x0=P, xt=P, nz=P, coef=P, mm=0, vm=2, vb=P, xm=P, ms=P, out_ld=1, group=2, B=2, n=64):
        return lib.vaw_bpd_terms(mean, var, ld, x0, xt, nz, coef, mm, vm, 1, vb, xm, ms, out_ld, group, B, n, None)

    for kw, word in ((dict(n=0), "sizes"), (dict(n=-4), "sizes"), (dict(B=0), "sizes"), (dict(mean=None), "null"), (dict(x0=None), "null"),
                     (dict(xt=None), "null"), (dict(nz=None), "null"), (dict(coef=None), "null"), (dict(vb=None), "null"),
                     (dict(ms=None), "null"), (dict(var=None), "modes"), (dict(vm=3), "modes"), (dict(vm=-1), "modes"),
                     (dict(mm=2), "modes"), (dict(ld=32), "model_ld"), (dict(group=0), "layout"), (dict(group=3, B=4), "layout"),
                     (dict(group=1, B=4, out_ld=2), "layout")):
        assert bpd(**kw) == -1, kw
        assert word in lib.vaw_last_error_string().decode(), (kw, lib.vaw_last_error_string())
    assert lib.vaw_prior_bpd(P, 0.1, -0.1, P, 2, 0, None) == -1 and "sizes" in lib.vaw_last_error_string().decode()
    assert lib.vaw_prior_bpd(None, 0.1, -0.1, P, 2, 64, None) == -1 and "null" in lib.vaw_last_error_string().decode()

    def ddim_reverse(mean=P, ld=64, x=P, n=64):          # kind 3 of the one reverse-step entry: no guidance, noise or variance
        return lib.vaw_guided_sample_step(3, mean, None, None, None, ld, 1.0, x, None, P, 0, 0, 1, 0.0, P, P, None, None, 2, n, None)

    assert ddim_reverse(n=0) == -1 and "sizes" in lib.vaw_last_error_string().decode()
    assert ddim_reverse(x=None) == -1 and "null" in lib.vaw_last_error_string().decode()
    assert ddim_reverse(ld=32) == -1 and "model_ld" in lib.vaw_last_error_string().decode()

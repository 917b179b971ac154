"""flow_log_likelihood on the GPU: vaw_flow_logp_stage / vaw_flow_logp_prior against the float32 tensor composition (state
bitwise; the float64 divergence to the rounding of a different summation order), their repeatability, and the whole evaluation
with the HIP DiT / UNet against the float64 restatement (tests/flow_logp_cases.py) driving the float64 oracle model.
Run on the MI355X box: pytest -m gpu."""
import math

import numpy as np
import pytest
import torch

from conftest import base_args, load_pt, perturb_

pytestmark = pytest.mark.gpu

import flow_logp_cases as fc
import vaw_amd
from oracle import diffusion as od
from oracle import dit as odit
from oracle import unet as ounet
from vaw_amd import ops, samplers

DEV = "cuda"


def _fm(mean_type, path="cosine"):
    return vaw_amd.FlowMatching(args=base_args(path_type=path), model_mean_type=vaw_amd.ModelMeanType[mean_type])


# ---- the kernels against the composition, one Runge-Kutta step at a time ---------------------------------------------------------
@pytest.mark.parametrize("solver", fc.SOLVERS)
@pytest.mark.parametrize("rows,shape,sigma", fc.KERNEL_CASES)
def test_stage_kernel_equals_composition(rows, shape, sigma, solver):
    """One step of `solver` from random x with random network outputs and vector-Jacobian products: every k slot, every stage
    state and x_new bitwise the float32 composition; every divergence row within 1e-12 * sum |eps * g| of the float64
    composition (the products are exact in float64, only the order of the sum differs), the accumulator likewise."""
    c, a, b = samplers._LOGP_TABLEAUS[solver]
    S, n, h = len(c), int(np.prod(shape)), 0.37
    g = torch.Generator().manual_seed(rows * 1000 + n + S)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x = rnd(rows, *shape)
    eps = (torch.randint(0, 2, (rows, *shape), generator=g).float() * 2 - 1).to(DEV)
    outs = [rnd(rows, (2 if sigma else 1) * shape[0], *shape[1:]) for _ in range(S)]
    gs = [rnd(rows, *shape) for _ in range(S)]
    ab = [(float(np.float32(0.3 + 0.2 * i)), float(np.float32(-1.1 + 0.4 * i))) for i in range(S)]
    coef = torch.tensor([[A, B, 0.0, 0.0] for A, B in ab], dtype=torch.float32, device=DEV)
    k = torch.full((ops.RK_STAGES, rows, *shape), float("nan"), device=DEV)
    d = torch.full((ops.RK_STAGES, rows), float("nan"), dtype=torch.float64, device=DEV)
    delta0 = torch.randn(rows, generator=g, dtype=torch.float64).to(DEV)
    delta = delta0.clone()
    count = ops.rk_partial_count(rows, n)
    assert count == rows * min(64, -(-n // 1024))
    partials = torch.full((count + 3,), 7.0, dtype=torch.float64, device=DEV) if n > 1024 else None
    guard = torch.full((rows + 2, *shape), 5.0, device=DEV)          # x_out sits between two canary rows
    bufs = [x] + [torch.empty_like(x) for _ in range(S - 1)] + [guard[1:rows + 1]]
    ks, ds, mags, states = [], [], [], [x]
    for i in range(S):
        last = i == S - 1
        coeffs = b if last else a[i + 1]
        out = outs[i][:, : shape[0]]
        ops.flow_logp_stage(i, out, gs[i], eps, x, bufs[i] if i else None, coef, i, k, d, coeffs, h, x_out=bufs[i + 1],
                            delta=delta if last else None, partials=partials)
        A, B = ab[i]
        ks.append(A * states[i] + B * out)
        prod = eps.double() * gs[i].double()
        ds.append(A * n + B * prod.flatten(1).sum(1))
        mags.append(prod.abs().flatten(1).sum(1))
        states.append(x + h * samplers._rk_combine(coeffs, ks))
        assert torch.equal(k[i], ks[i]), (i, "k")
        assert torch.equal(bufs[i + 1], states[i + 1]), (i, "state")
        err = (d[i] - ds[i]).abs()
        assert bool((err <= 1e-12 * mags[i]).all()), (i, err.tolist(), mags[i].tolist())
    want = delta0 + h * samplers._rk_combine(b, ds)
    allowed = 1e-12 * torch.stack(mags).amin(0)          # the smallest sum |eps * g| among the step's stages, per row
    assert bool(((delta - want).abs() <= allowed).all()), ((delta - want).abs().tolist(), allowed.tolist())
    assert bool((guard[0] == 5.0).all()) and bool((guard[-1] == 5.0).all())          # nothing outside x_out
    assert torch.isnan(k[S:]).all() and torch.isnan(d[S:]).all()                     # nor in the slots of other stages
    if partials is not None:
        assert bool((partials[count:] == 7.0).all())
    # the prior of the step's end state
    z = bufs[S].contiguous()
    want = fc.gaussian_logp(z)
    got = ops.flow_logp_prior(z)
    assert got.dtype == torch.float64 and bool(((got - want).abs() <= 1e-12 * (z.double() ** 2).flatten(1).sum(1)).all())


def test_stage_kernel_refuses_bad_arguments():
    x = torch.zeros(2, 8, device=DEV)
    k, d = torch.zeros(ops.RK_STAGES, 2, 8, device=DEV), torch.zeros(ops.RK_STAGES, 2, dtype=torch.float64, device=DEV)
    coef = torch.zeros(2, ops.FLOW_LOGP_COLS, device=DEV)
    good = dict(x_out=torch.zeros(2, 8, device=DEV))
    ops.flow_logp_stage(0, x, x, x, x, None, coef, 1, k, d, (1.0,), 0.1, **good)
    for bad in (lambda: ops.flow_logp_stage(0, x, x, x, x, None, coef, 2, k, d, (1.0,), 0.1, **good),                  # row outside
                lambda: ops.flow_logp_stage(7, x, x, x, x, None, coef, 0, k, d, (1.0,), 0.1, **good),                  # stage outside
                lambda: ops.flow_logp_stage(0, x, x, x, x, None, coef, 0, k, d, (1.0,) * 8, 0.1, **good),              # too many weights
                lambda: ops.flow_logp_stage(0, x, x, x, x, None, coef, 0, k, d, (1.0,), 0.1, x_out=x),                 # overlap
                lambda: ops.flow_logp_stage(0, x, x, x, x, None, coef, 0, k, d, (1.0,), 0.1),                          # no x_out
                lambda: ops.flow_logp_stage(0, x, x, x, x, None, coef, 0, k[:, :1], d, (1.0,), 0.1, **good),           # k too small
                lambda: ops.flow_logp_stage(0, x, x, x.double(), x, None, coef, 0, k, d, (1.0,), 0.1, **good),         # dtype
                lambda: ops.flow_logp_stage(0, x, x, x, x, None, torch.zeros(2, 16, device=DEV), 0, k, d, (1.0,), 0.1, **good)):
        with pytest.raises(vaw_amd.VawError):
            bad()
    big = torch.zeros(1, 4100, device=DEV)
    with pytest.raises(vaw_amd.VawError):          # a row of five workgroups needs its partial sums
        ops.flow_logp_stage(0, big, big, big, big, None, coef, 0, torch.zeros(ops.RK_STAGES, 1, 4100, device=DEV),
                            torch.zeros(ops.RK_STAGES, 1, dtype=torch.float64, device=DEV), (1.0,), 0.1, x_out=torch.zeros_like(big))


# ---- the whole evaluation with a stand-in model ---------------------------------------------------------------------------------------
def _standin_run(monkeypatch, rows, shape, sigma, solver, mean_type, probes, fused, K=1, record=None):
    model = fc.Standin(shape[0], sigma=sigma).to(DEV).eval()
    x = torch.randn(3, *shape, generator=torch.Generator().manual_seed(31))[:rows].contiguous().to(DEV)          # row i is row i of any batch
    monkeypatch.setattr(samplers, "_logp_probes", lambda kind, shp, dtype, device, gen: probes.to(device))
    if record is not None:
        inner = samplers._logp_network

        def spy(model, xin, t_rows, eps, kw):
            out, g = inner(model, xin, t_rows, eps, kw)
            record.append(float((eps.double() * g.double()).abs().flatten(1).sum(1).max()))
            return out, g
        monkeypatch.setattr(samplers, "_logp_network", spy)
    r = _fm(mean_type).calc_bpd(model, x, num_steps=4, solver=solver, t_span=fc.regular_span(mean_type), n_probes=K, fused=fused)
    monkeypatch.undo()
    return r


def _probes(rows, shape, seed=41):
    return torch.randint(0, 2, (rows, *shape), generator=torch.Generator().manual_seed(seed)).float() * 2 - 1


@pytest.mark.parametrize("solver,mean_type", [("euler", "VECTOR"), ("heun", "VELOCITY"), ("rk4", "START_X"), ("heun", "EPSILON")])
@pytest.mark.parametrize("rows,shape,sigma", fc.KERNEL_CASES)
def test_fused_equals_composition_with_standin(monkeypatch, rows, shape, sigma, solver, mean_type):
    p = _probes(rows, shape)
    mags = []
    comp = _standin_run(monkeypatch, rows, shape, sigma, solver, mean_type, p, False, record=mags)
    fused = _standin_run(monkeypatch, rows, shape, sigma, solver, mean_type, p, None)
    assert fused["z"].dtype == torch.float32 and torch.equal(fused["z"], comp["z"])
    tab = samplers._flow_logp_tables(_fm(mean_type), solver, 4, fc.regular_span(mean_type))
    allowed = 1e-12 * min(mags)          # the smallest sum |eps * g| (largest row) among the call's evaluations
    err = float((fused["delta_logp"] - comp["delta_logp"]).abs().max())
    assert err <= allowed, (err, allowed)
    n = int(np.prod(shape))
    perr = float((fused["prior_logp"] - comp["prior_logp"]).abs().max())
    assert perr <= 1e-12 * float((comp["z"].double() ** 2).flatten(1).sum(1).max()), perr
    assert fused["nfev"] == comp["nfev"] == len(tab.times) and fused["logp"].dtype == torch.float64
    torch.testing.assert_close(fused["bpd"], -fused["logp"] / (n * math.log(2.0)), rtol=1e-15, atol=0)


@pytest.mark.parametrize("shape", [(3, 5, 5), (3, 8, 8), (4, 25, 41)])
def test_repeatable_and_independent_of_the_batch(monkeypatch, shape):
    p = _probes(3, shape)
    run = lambda rows, probes, K=1: _standin_run(monkeypatch, rows, shape, False, "heun", "VELOCITY", probes, None, K=K)
    a, b = run(3, p), run(3, p)
    for key in ("logp", "delta_logp", "prior_logp", "z"):
        assert torch.equal(a[key], b[key]), key
    # row 0 alone
    alone = run(1, p[:1])
    for key in ("logp", "delta_logp", "prior_logp", "z"):
        assert torch.equal(alone[key], a[key][:1]), key
    # two probes stacked on the batch axis = the float64 mean of the two single-probe runs
    q = _probes(3, shape, seed=43)
    two, one = run(3, torch.cat((p, q)), K=2), run(3, q)
    assert torch.equal(two["delta_logp"], (a["delta_logp"] + one["delta_logp"]) / 2)
    assert torch.equal(two["z"], a["z"]) and torch.equal(two["prior_logp"], a["prior_logp"]) and two["nfev"] == a["nfev"]


def test_fused_true_refuses_float64_on_the_gpu():
    model = fc.Standin(3, dtype=torch.float64).to(DEV).eval()
    x = torch.zeros(2, 3, 4, 4, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="float64"):
        vaw_amd.flow_log_likelihood(_fm("VELOCITY"), model, x, num_steps=3, fused=True)
    r = vaw_amd.flow_log_likelihood(_fm("VELOCITY"), model, x, num_steps=3)          # fused=None: the composition
    assert r["z"].dtype == torch.float64 and torch.isfinite(r["logp"]).all()


# ---- end to end: the HIP models against the float64 oracle ------------------------------------------------------------------------------
def _sinusoid64(t, dim, max_period=10000):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=t.dtype) / half)
    ang = t[:, None] * freqs[None]
    emb = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1)
    return torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1) if dim % 2 else emb


def _attend64(q, k, v, ch):
    s = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v)


def _native_dtype_oracle(monkeypatch):
    """The oracle models pin three pieces to float32 (the timestep embedding, the UNet's GroupNorm and its softmax); for the
    float64 run they follow the input's dtype instead, so that the float64 oracle is float64 throughout."""
    monkeypatch.setattr(odit, "sinusoid", _sinusoid64)
    monkeypatch.setattr(ounet, "timestep_embedding", _sinusoid64)
    monkeypatch.setattr(ounet, "_attend", _attend64)
    monkeypatch.setattr(ounet.GroupNorm32, "forward", torch.nn.GroupNorm.forward)


def _models(kind, dtype):
    if kind == "dit":
        g = load_pt("dit_tiny.pt")
        kw = dict(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, **g["p2/kw"])
        torch.manual_seed(11)
        hip = vaw_amd.DiT(compute_dtype=dtype, **kw)
        perturb_(hip, 99)
        oracle = odit.DiT(**kw)
        x, y = g["p2/x"], g["p2/y"]
    else:
        g = load_pt("unet_tiny.pt")
        kw = g["new/kw"]
        torch.manual_seed(21)
        hip = vaw_amd.UNetModel(compute_dtype=dtype, **kw)
        perturb_(hip, 77, std=0.03)
        oracle = ounet.UNetModel(**kw)
        x, y = g["new/x"], (g["new/y"] if g["new/y"].numel() else None)
    oracle.load_state_dict({k: v.detach().clone() for k, v in hip.state_dict().items()})
    return hip.to(DEV).eval(), oracle.eval(), x, ({} if y is None else {"y": y})


class _Autocast(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x, t, **kw):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = self.model(x, t, **kw)
        out = out[0] if isinstance(out, tuple) else out
        return out.float()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["dit", "unet"])
def test_end_to_end_against_float64_oracle(monkeypatch, kind, dtype):
    """logp of the HIP model (fused kernels, input_grad_only backward) against the float64 restatement driving the float64 oracle
    with the same weights, x and probes.  The allowance calibrates itself: e_ref = |oracle in the HIP model's precision - oracle
    in float64| on this very case (float32 tensor composition on the CPU; for bf16 the same under CPU bf16 autocast), and
    |HIP - oracle64| <= 4 e_ref, the project's usual factor for another summation order and fast transcendentals."""
    hip, oracle, x, kw = _models(kind, dtype)
    fm, ofm = _fm("VELOCITY"), od.FlowMatching(args=base_args(path_type="cosine"), model_mean_type=od.ModelMeanType.VELOCITY)
    N, steps, solver = x.shape[0], 4, "heun"
    probes = _probes(N, tuple(x.shape[1:]), seed=47)
    monkeypatch.setattr(samplers, "_logp_probes", lambda kind_, shp, dt, device, gen: probes.to(device))
    low = fm.calc_bpd(_Autocast(oracle).eval() if dtype == "bf16" else oracle, x, num_steps=steps, solver=solver, fused=False, **kw)
    got = fm.calc_bpd(hip, x.to(DEV), num_steps=steps, solver=solver, **{k: v.to(DEV) for k, v in kw.items()})
    assert hip._flat_grad is None and all(p.grad is None for p in hip.parameters())          # the evaluation grew no gradients
    _native_dtype_oracle(monkeypatch)
    ref = fc.restate(ofm, oracle.double(), x.double(), probes.double()[None], (0.0, 1.0), steps, solver, **kw)
    e_ref = float((low["logp"] - ref["logp"]).abs().max())
    err = float((got["logp"].cpu() - ref["logp"]).abs().max())
    print(f"flow logp {kind} {dtype}: |HIP - oracle64| = {err:.3e}, e_ref = {e_ref:.3e}, err / allowed = {err / (4 * e_ref):.3f}, "
          f"logp ~ {float(ref['logp'].abs().mean()):.3f}")
    assert torch.isfinite(got["logp"]).all() and got["nfev"] == got["nvjp"] == 6
    assert err <= 4 * e_ref, (err, e_ref)

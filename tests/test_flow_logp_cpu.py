"""flow_log_likelihood on the CPU: the conventions of the float64 restatement (tests/flow_logp_cases.py) against an independent
integrator and a closed form, the collapsed field coefficients against the reference's conversion, the tensor composition
(fused=False) against the restatement, and every refusal.  No kernel is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, base_args

import flow_logp_cases as fc
import abi_cases
import vaw_amd
from oracle import diffusion as od
from vaw_amd import samplers


def _fm(mean_type, path="cosine"):
    return vaw_amd.FlowMatching(args=base_args(path_type=path), model_mean_type=vaw_amd.ModelMeanType[mean_type])


def _ofm(mean_type, path="cosine"):
    return od.FlowMatching(args=base_args(path_type=path), model_mean_type=od.ModelMeanType[mean_type])


# ---- 1. conventions against an independent integrator -----------------------------------------------------------------------------
def test_restatement_converges_to_dop853_with_the_solvers_order():
    """v = tanh(W x + b t) on 6 dimensions, exact divergence sum (1 - u^2) diag W.  Reference: scipy DOP853 at rtol = atol =
    1e-13 on the augmented system.  Measured with W ~ 0.7 N(0, 1) from default_rng(0), error on the integral at 17 / 33 / 65
    grid points: euler 3.4e-2 / 1.7e-2 / 8.5e-3, heun 7.5e-4 / 1.9e-4 / 4.8e-5, rk4 3.9e-8 / 3.1e-9 / 2.1e-10 (state at 65: 9.6e-10)."""
    from scipy.integrate import solve_ivp
    rng = np.random.default_rng(0)
    W, b, x0 = 0.7 * rng.standard_normal((6, 6)), rng.standard_normal(6), rng.standard_normal(6)

    def rhs(t, s):
        u = np.tanh(W @ s[:6] + b * t)
        return np.concatenate([u, [np.sum((1 - u ** 2) * np.diag(W))]])

    ref = solve_ivp(rhs, (0.0, 1.0), np.concatenate([x0, [0.0]]), method="DOP853", rtol=1e-13, atol=1e-13).y[:, -1]
    Wt, bt = torch.from_numpy(W), torch.from_numpy(b)

    def field_div(x, t):
        u = torch.tanh(x @ Wt.T + bt * t)
        return u, ((1 - u ** 2) * torch.diagonal(Wt)).sum(1)

    order = {"euler": 1, "heun": 2, "rk4": 4}
    for solver, p in order.items():
        errs = []
        for pts in (17, 33, 65):
            r = fc.integrate(field_div, torch.from_numpy(x0)[None], np.linspace(0.0, 1.0, pts), solver)
            errs.append((abs(float(r["delta_logp"][0]) - ref[6]), float(np.abs(r["z"][0].numpy() - ref[:6]).max())))
        print(solver, errs)
        for coarse, fine in zip(errs, errs[1:]):
            ratio = coarse[0] / fine[0]
            assert 0.7 * 2 ** p <= ratio <= 1.4 * 2 ** p, (solver, errs)
    assert errs[-1][0] < 1e-8 and errs[-1][1] < 1e-8, errs          # rk4 at 65 points: integral and state
    prior = fc.gaussian_logp(torch.from_numpy(ref[:6])[None])
    assert abs(float(r["logp"][0]) - (float(prior[0]) + ref[6])) < 2e-8


# ---- 2. closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", ["rademacher", "gaussian"])
def test_linear_vector_field_closed_form(probe):
    """VECTOR with v = diag(w) x:  x(1) = e^w x0 and log p0(x0) = log N(e^w x0; 0, I) + sum w.  Rademacher probes are exact for
    a diagonal Jacobian (eps^2 = 1); Gaussian ones are not, and only have to leave the state and the prior alone."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(7, generator=g, dtype=torch.float64) * 0.5
    x0 = torch.randn(4, 7, generator=g, dtype=torch.float64)
    r = vaw_amd.flow_log_likelihood(_fm("VECTOR"), lambda x, t, **_: x * w, x0, num_steps=65, solver="rk4", probe=probe,
                                    generator=torch.Generator().manual_seed(1), fused=False)
    z = x0 * torch.exp(w)
    assert float((r["z"] - z).abs().max()) < 1e-8 and r["z"].dtype == torch.float64
    assert float((r["prior_logp"] - fc.gaussian_logp(z)).abs().max()) < 1e-8
    for k in ("logp", "prior_logp", "delta_logp", "bpd"):
        assert r[k].dtype == torch.float64 and r[k].shape == (4,)
    assert r["nfev"] == r["nvjp"] == 64 * 4
    if probe == "rademacher":
        assert float((r["logp"] - (fc.gaussian_logp(z) + w.sum())).abs().max()) < 1e-8
        assert float((r["delta_logp"] - w.sum()).abs().max()) < 1e-8
        torch.testing.assert_close(r["bpd"], -r["logp"] / (7 * math.log(2.0)), rtol=1e-15, atol=0)
        off = vaw_amd.flow_log_likelihood(_fm("VECTOR"), lambda x, t, **_: x * w, x0, num_steps=5, solver="euler", fused=False, offset_bits=7.0)
        torch.testing.assert_close(off["bpd"], -off["logp"] / (7 * math.log(2.0)) + 7.0, rtol=1e-15, atol=0)
    else:
        assert float((r["delta_logp"] - w.sum()).abs().max()) > 1e-3


# ---- 3. A / B per mean type and path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", fc.PATHS)
@pytest.mark.parametrize("mean_type", fc.MEAN_TYPES)
def test_collapsed_coefficients_equal_the_reference_conversion(mean_type, path):
    g = torch.Generator().manual_seed(17)
    out, x = torch.randn(2, 5, generator=g, dtype=torch.float64), torch.randn(2, 5, generator=g, dtype=torch.float64)
    ofm = _ofm(mean_type, path)
    for t in (0.07, 0.31, 0.5, 0.83, 0.96):
        A, B = samplers._flow_logp_ab(_fm(mean_type, path), t)
        ref = fc.reference_vector(ofm.interpolant, mean_type, out, x, torch.full((2, 1), t, dtype=torch.float64))
        got = A * x + B * out
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (mean_type, path, t)


# ---- 4. the tensor composition in float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", fc.SOLVERS)
@pytest.mark.parametrize("mean_type,path,sigma,K", [("VELOCITY", "cosine", False, 1), ("START_X", "linear", False, 2),
                                                    ("EPSILON", "linear_logsnr", True, 1), ("VECTOR", "linear", True, 2)])
def test_composition_float64_equals_restatement(solver, mean_type, path, sigma, K):
    N, shape = 3, (3, 4, 5)
    g = torch.Generator().manual_seed(23)
    x0 = torch.randn(N, *shape, generator=g, dtype=torch.float64)
    model = fc.Standin(3, sigma=sigma, dtype=torch.float64).eval()
    span = fc.regular_span(mean_type)
    r = _fm(mean_type, path).calc_bpd(model, x0, num_steps=6, solver=solver, t_span=span, n_probes=K, fused=False,
                                      generator=torch.Generator().manual_seed(9))
    probes = samplers._logp_probes("rademacher", (K * N, *shape), torch.float64, x0.device, torch.Generator().manual_seed(9))
    assert set(probes.unique().tolist()) == {-1.0, 1.0}
    ref = fc.restate(_ofm(mean_type, path), model, x0, probes.view(K, N, *shape), span, 6, solver)
    for k in ("z", "delta_logp", "prior_logp", "logp"):
        scale = float(ref[k].abs().max())
        assert float((r[k] - ref[k]).abs().max()) <= 1e-12 * scale, (k, float((r[k] - ref[k]).abs().max()), scale)


def test_probes_are_drawn_once_and_fixed():
    """One draw per call from `generator`: the same seed gives the same result, another seed another estimate, and the state
    does not depend on the probes at all."""
    x0 = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    model, fm = fc.Standin(3, dtype=torch.float64).eval(), _fm("VELOCITY")
    run = lambda seed, **kw: fm.calc_bpd(model, x0, num_steps=4, solver="heun", fused=False, generator=torch.Generator().manual_seed(seed), **kw)
    a, b, c = run(1), run(1), run(2)
    assert torch.equal(a["logp"], b["logp"]) and not torch.equal(a["logp"], c["logp"]) and torch.equal(a["z"], c["z"])
    gauss = run(1, probe="gaussian")
    assert torch.equal(gauss["z"], a["z"]) and not torch.equal(gauss["delta_logp"], a["delta_logp"])


# ---- 5. refusals, CPU wrappers, symbols -------------------------------------------------------------------------------------------------
def test_refusals_come_with_the_reason():
    x = torch.zeros(2, 3, 4, 4)
    plain = fc.Standin(3).eval()
    call = lambda fm=_fm("VELOCITY"), model=plain, x=x, **kw: vaw_amd.flow_log_likelihood(fm, model, x, num_steps=3, **kw)
    with pytest.raises(ValueError, match="training mode"):
        call(model=fc.Standin(3).train())
    cfg = vaw_amd.IntervalCFG(plain, 10, guidance_scale=2.0, interval=(0.2, 0.8)).eval()
    with pytest.raises(ValueError, match="guided field"):
        call(model=cfg, y=torch.zeros(2, dtype=torch.long))
    # the same wrapper with guidance off for good, or without labels, passes through to the wrapped model
    seeded = lambda: dict(fused=False, generator=torch.Generator().manual_seed(4))
    off = call(model=vaw_amd.IntervalCFG(plain, 10, guidance_scale=1.0).eval(), y=torch.zeros(2, dtype=torch.long), **seeded())
    assert torch.equal(off["logp"], call(**seeded())["logp"])
    assert torch.isfinite(call(model=cfg, fused=False)["logp"]).all()
    with pytest.raises(ValueError, match="SCORE"):
        call(fm=_fm("SCORE"))
    for solver in ("rk45", "dopri5"):
        with pytest.raises(ValueError, match="adaptive control"):
            call(solver=solver)
    with pytest.raises(ValueError, match="unknown solver"):
        call(solver="midpoint")
    with pytest.raises(ValueError, match=r"EPSILON.*'linear'.*t=1\.0"):
        call(fm=_fm("EPSILON", "linear"))
    with pytest.raises(ValueError, match=r"START_X.*t=0\.0"):
        call(fm=_fm("START_X", "cosine"))
    assert torch.isfinite(call(fm=_fm("START_X", "cosine"), t_span=(0.1, 1.0), fused=False)["logp"]).all()
    with pytest.raises(ValueError, match="fused=True"):
        call(fused=True)                                      # CPU tensors
    with pytest.raises(ValueError, match="n_probes"):
        call(n_probes=0)
    with pytest.raises(ValueError, match="probe"):
        call(probe="sphere")
    fp8 = fc.Standin(3).eval()
    fp8.compute_dtype = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        call(model=fp8)
    with pytest.raises(ValueError, match="fp8"):
        call(model=vaw_amd.IntervalCFG(fp8, 10).eval())


def test_refusals_precede_the_model_call():
    def never(*a, **k):
        raise AssertionError("the model was called")
    for kw in (dict(solver="rk45"), dict(n_probes=0), dict(fm=_fm("EPSILON", "linear")), dict(fm=_fm("SCORE"))):
        fm = kw.pop("fm", _fm("VELOCITY"))
        with pytest.raises(ValueError):
            vaw_amd.flow_log_likelihood(fm, never, torch.zeros(1, 2), num_steps=3, **kw)


def test_input_grad_only_is_declared_on_flat_module_and_refuses_fp8():
    assert hasattr(vaw_amd.FlatModule, "input_grad_only")
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=1, num_heads=2, num_classes=10, compute_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        with m.input_grad_only():
            pass
    with pytest.raises(ValueError, match="fp8"):
        vaw_amd.flow_log_likelihood(_fm("VELOCITY"), m.eval(), torch.zeros(2, 4, 8, 8), num_steps=3)
    u = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=1, num_heads=2, num_classes=10)
    assert u._input_grad_only is False
    with u.input_grad_only() as inner:
        assert inner is u and u._input_grad_only is True
        with u.input_grad_only():
            pass
        assert u._input_grad_only is True
    assert u._input_grad_only is False


def test_cpu_wrappers_refuse_and_symbols_are_bound():
    x = torch.zeros(2, 8)
    k, d = torch.zeros(vaw_amd.ops.RK_STAGES, 2, 8), torch.zeros(vaw_amd.ops.RK_STAGES, 2, dtype=torch.float64)
    coef = torch.zeros(1, vaw_amd.ops.FLOW_LOGP_COLS)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.flow_logp_stage(0, x, x, x, x, None, coef, 0, k, d, (1.0,), 0.1, x_out=torch.zeros(2, 8))
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.flow_logp_prior(x)
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    assert int(re.search(r"#define VAW_FLOW_LOGP_COLS (\d+)", hdr).group(1)) == vaw_amd.ops.FLOW_LOGP_COLS
    assert int(re.search(r"#define VAW_FLOW_COLS (\d+)", hdr).group(1)) == 16          # the samplers' table is left alone
    lib = vaw_amd.lib()
    for name in ("vaw_flow_logp_stage", "vaw_flow_logp_prior"):
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        bound = abi_cases.assert_bound_as_declared(lib, name)          # every parameter as the header's prototype spells it
        assert sum(b is ctypes.c_double for b in bound) == (1 if name.endswith("stage") else 0)          # h alone goes by value as a double
    assert lib.vaw_flow_logp_stage.argtypes[12] == ctypes.POINTER(ctypes.c_double)          # a_host: the host array of coefficients

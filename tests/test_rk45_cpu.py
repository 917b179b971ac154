"""flow_ode_sample(solver="rk45") on the CPU: the float32 tensor composition of the adaptive Dormand-Prince 5(4) solver against
the float64 scipy fixture (tests/golden/rk45.npz) and a live solve_ivp, the step controller on closed-form drifts, the ends
that raise, tolerance resolution, refusals, and the C entry points' argument checks."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rk45_cases as rc
import abi_cases
import vaw_amd
from conftest import GOLDEN
from vaw_amd import ops, samplers

FIX = np.load(os.path.join(GOLDEN, "rk45.npz"))


def run_case(case, **kw):
    path, mean, shape = case
    x0, y = rc.inputs(shape)
    fm = rc.flow(path, mean)
    got = vaw_amd.flow_ode_sample(fm, rc.standin, x0, solver="rk45", rtol=rc.RTOL, atol=rc.ATOL, y=y, **kw)
    return x0, y, got, fm.last_ode_stats


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_composition_reproduces_the_scipy_fixture(case):
    cid = rc.case_id(case)
    x0, y, got, st = run_case(case)
    assert np.array_equal(x0.numpy(), FIX[f"{cid}/x0"]) and np.array_equal(y.numpy(), FIX[f"{cid}/y"])
    assert got.dtype == torch.float32 and got.shape == x0.shape
    attempts = st["accepted"] + st["rejected"]
    assert (st["accepted"], attempts) == (int(FIX[f"{cid}/accepted"]), int(FIX[f"{cid}/attempts"])), st
    assert st["nfev"] == 2 + 6 * attempts + 1 == int(FIX[f"{cid}/nfev"]) + 1 and st["readbacks"] <= attempts + 2
    diff = float(np.abs(got.double().numpy() - FIX[f"{cid}/final"]).max())
    print(f"{cid}: max |diff| vs the fixture {diff:.3e}, recorded {float(FIX[f'{cid}/dist']):.3e}")
    assert diff <= 2 * float(FIX[f"{cid}/dist"])          # (2: libm differences between builds; nothing else differs)
    assert len(st["trace"]) == attempts and 0 < st["h_min"] <= st["h_max"] <= 1
    assert not any(0.69 < n < 1.26 for _, _, n in st["trace"]), "an error ratio an ulp of drift could move across 1"


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_composition_reproduces_a_live_solve_ivp(case):
    pytest.importorskip("scipy")
    cid = rc.case_id(case)
    x0, y, got, st = run_case(case, fused=False)
    final, nfev, attempts, accepted = rc.scipy_run(case[0], case[1], x0, y)
    assert (st["accepted"], st["accepted"] + st["rejected"], st["nfev"]) == (accepted, attempts, nfev + 1)
    assert float(np.abs(got.double().numpy() - final).max()) <= 2 * float(FIX[f"{cid}/dist"])


# ---- the controller, on scalar closed-form drifts (VECTOR: the model output is the drift) -------------------------------------
def vector_fm(**extra):
    return rc.flow("linear", "VECTOR", **extra)


def integrate(drift, x0=1.0, **kw):
    fm = vector_fm()
    x = vaw_amd.flow_ode_sample(fm, lambda x, t, **_: drift(x, t.view(-1, 1)), torch.full((1, 1), x0), solver="rk45", **kw)
    return float(x), fm.last_ode_stats


def test_zero_error_grows_the_step_tenfold_and_the_last_step_lands_on_the_end():
    x, st = integrate(lambda x, t: torch.zeros_like(x))          # d1 = d2 = 0: h0 = h1 = 1e-6; every error ratio is exactly 0
    assert x == 1.0 and st["rejected"] == 0
    trace = st["trace"]
    assert trace[0][0] == 1.0 and trace[0][1] == pytest.approx(-1e-6, rel=1e-9) and all(n == 0 for _, _, n in trace)
    for (t0, h0, _), (t1, h1, _) in zip(trace[:-2], trace[1:-1]):
        assert t1 == t0 + h0 and abs(h1) == pytest.approx(10 * abs(h0), rel=1e-9)          # (h = t_new - t: to the rounding of t)
    t_last, h_last, _ = trace[-1]
    assert t_last + h_last == 0.0 and abs(h_last) < 10 * abs(trace[-2][1])          # clipped, and exactly on t = 0
    assert st["nfev"] == 2 + 6 * len(trace) + 1 and st["h_max"] == max(abs(h) for _, h, _ in trace)


def test_factor_is_capped_at_one_after_a_rejection():
    # dx/dt = [t < 0.5]: zero error until a step straddles t = 0.5, which is rejected; the shortened step that stops short of the
    # jump has zero error again (factor 10 without the cap), so the step after it must be exactly as long
    x, st = integrate(lambda x, t: (t < 0.5).to(x.dtype).expand_as(x), rtol=1e-3, atol=1e-6)
    trace = st["trace"]
    assert st["rejected"] > 0
    checked = 0
    for i in range(1, len(trace) - 1):
        (tp, hp, n_prev), (t, h, n), (tn, hn, _) = trace[i - 1], trace[i], trace[i + 1]
        if n_prev >= 1 and n == 0 and tn + hn != 0.0:          # accepted with zero error right after a rejection, next not clipped
            assert tn == t + h and abs(hn) == pytest.approx(abs(h), rel=1e-12), (trace[i - 1:i + 2])
            checked += 1
    assert checked > 0, trace
    assert trace[-1][0] + trace[-1][1] == 0.0
    # x(0) = x(1) - integral of the drift = 0.5, loosely: the error estimate assumes a smooth drift, and a step whose stages all
    # but the last lie before the jump passes it
    assert x == pytest.approx(0.5, abs=0.02)


def test_smooth_scalar_ode_meets_its_tolerance():
    x, st = integrate(lambda x, t: -2 * t * x, rtol=1e-5, atol=1e-7)          # x(t) = x(1) exp(1 - t^2)
    assert x == pytest.approx(math.e, rel=1e-4) and st["accepted"] > 3


def test_nan_model_raises_floating_point_error_within_one_attempt():
    calls = []

    def model(x, t, **_):
        calls.append(float(t[0]))
        return torch.full_like(x, math.nan)

    with pytest.raises(FloatingPointError, match=r"t=1\.0"):
        vaw_amd.flow_ode_sample(vector_fm(), model, torch.ones(2, 3), solver="rk45")
    assert len(calls) <= 2 + 7

    def late(x, t, **_):          # finite through the first-step selection, NaN in the step: the error norm names t and h
        calls.append(float(t[0]))
        return torch.full_like(x, math.nan if len(calls) > 12 else 1.0)

    del calls[:]
    with pytest.raises(FloatingPointError, match=r"error norm at t=.*h=-"):
        vaw_amd.flow_ode_sample(vector_fm(), late, torch.ones(2, 3), solver="rk45")
    assert len(calls) <= 12 + 6


def test_max_attempts_raises_runtime_error():
    fm = vector_fm()
    with pytest.raises(RuntimeError, match="max_attempts=3"):
        vaw_amd.flow_ode_sample(fm, lambda x, t, **_: torch.sin(40 * t.view(-1, 1)) * x, torch.ones(1, 4), solver="rk45", rtol=1e-6,
                                atol=1e-8, max_attempts=3)
    assert fm.last_ode_stats["accepted"] + fm.last_ode_stats["rejected"] == 3


def test_step_below_the_spacing_of_t_raises_runtime_error():
    # a tolerance no float32 stage can meet (rtol = 0, atol at the bottom of the float32 range): every attempt is rejected and
    # the step shrinks until it is below ten spacings of t
    fm = vector_fm()
    with pytest.raises(RuntimeError, match="below the spacing"):
        vaw_amd.flow_ode_sample(fm, lambda x, t, **_: torch.sin(3 * x) + t.view(-1, 1), torch.linspace(0.5, 2, 8).view(1, 8), solver="rk45",
                                rtol=0.0, atol=1e-37)
    st = fm.last_ode_stats
    assert st["accepted"] == 0 and 0 < st["rejected"] < 1000


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_tolerances_resolve_keyword_then_fm_then_args_then_defaults():
    fm = vector_fm()
    assert samplers._ode_tolerances(fm, None, None) == (1e-3, 1e-6)
    assert samplers._ode_tolerances(vector_fm(rtol=1e-2, atol=1e-4), None, None) == (1e-2, 1e-4)
    both = vector_fm(rtol=1e-2, atol=1e-4)
    both.rtol, both.atol = 1e-5, 1e-7
    assert samplers._ode_tolerances(both, None, None) == (1e-5, 1e-7)
    assert samplers._ode_tolerances(both, 1e-1, None) == (1e-1, 1e-7) and samplers._ode_tolerances(both, None, 0.5) == (1e-5, 0.5)
    # ... and reach the solver: a looser tolerance takes fewer attempts
    drift = lambda x, t, **_: -2 * t.view(-1, 1) * x
    counts = []
    for f in (vector_fm(rtol=1e-2, atol=1e-3), vector_fm(rtol=1e-7, atol=1e-8)):
        vaw_amd.flow_ode_sample(f, drift, torch.ones(1, 4), solver="rk45")
        counts.append(f.last_ode_stats["accepted"])
    assert counts[0] < counts[1]


def test_num_steps_is_ignored_and_other_entry_points_refuse():
    drift = lambda x, t, **_: -2 * t.view(-1, 1) * x
    x0 = torch.ones(1, 4)
    a = vaw_amd.flow_ode_sample(vector_fm(), drift, x0, num_steps=3, solver="rk45")
    b = vaw_amd.flow_ode_sample(vector_fm(), drift, x0, num_steps=500, solver="rk45")
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="Unknown solver"):
        vaw_amd.flow_sde_sample(vector_fm(), drift, x0, solver="rk45")
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.flow_ode_sample(vector_fm(), drift, x0, solver="rk45", fused=True)
    with pytest.raises(NotImplementedError, match="dopri5.*rk45"):
        vaw_amd.flow_ode_sample(vector_fm(), drift, x0, solver="dopri5")


def test_sampler_runs_rk45_and_refuses_hip_graph():
    from sampler_cases import Standin, sampler_args
    st = dict(guidance_scale=1.0, solver="rk45", path_type="linear", mean_type="VECTOR")
    model = Standin(lambda x, t, y=None, **kw: -2 * t.view(-1, 1, 1, 1) * x)
    args = sampler_args("flow", st, sampler_type="ode", rtol=1e-4, atol=1e-6)
    diff = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VECTOR)
    torch.manual_seed(5)
    images, labels = vaw_amd.Sampler(args, torch.device("cpu"), model, diff).sample(4, 2, 4, 10)
    assert len(images) == 2 and images[0].dtype.name == "uint8" and images[0].shape == (2, 4, 4, 3)
    assert diff.last_ode_stats["accepted"] > 0
    torch.manual_seed(5)          # the bytes of the composition called directly with args' tolerances
    y = torch.randint(0, 10, (2,))
    x = vaw_amd.flow_ode_sample(diff, model, torch.randn(2, 3, 4, 4), solver="rk45", rtol=1e-4, atol=1e-6, y=y)
    ref = ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert (images[0] == ref).all() and (labels[0] == y.numpy()).all()
    args = sampler_args("flow", st, sampler_type="ode", hip_graph=True, cpu_rng=False)
    with pytest.raises(ValueError, match="hip_graph.*rk45"):
        vaw_amd.Sampler(args, torch.device("cpu"), model, diff).sample(4, 2, 4, 10)


def test_rk_entry_points_have_argtypes_and_reject_bad_arguments_before_any_launch():
    import ctypes as C

    lib = vaw_amd.lib()
    for name, nargs in (("vaw_rk_stage", 26), ("vaw_rk_scaled_sumsq", 11), ("vaw_rk_sumsq_finish", 4)):
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        assert len(abi_cases.assert_bound_as_declared(lib, name)) == nargs
    assert "vaw_rk_partial_count" in vaw_amd.exported_symbols() and ops.RK_STAGES == 7
    with open(f"{vaw_amd.__path__[0]}/../include/vaw_hip.h") as f:
        header = f.read()
    assert "#define VAW_RK_STAGES 7" in header and "#define VAW_RK_MAX_GRID_X 64" in header
    # one partial sum per workgroup: a sample's row in 1024-element pieces, at most 64
    assert [ops.rk_partial_count(*a) for a in ((3, 75), (2, 256), (3, 4096), (1, 1024), (1, 1025), (2, 1 << 20), (0, 5))] == [3, 2, 12, 1, 2, 128, 0]
    p = 4096          # never dereferenced: every call below fails its argument check
    ident, coef = (C.c_int * 7)(*range(7)), (C.c_float * 7)(*([0.5] * 7))

    def stage(i=2, mt=2, c=p, u=p, ld=192, x=p, xs=p, tab=p, row=2, rows=7, k=p, slots=ident, a=coef, nc=3, xo=p, xn=None, part=None, cap=0,
              B=3, n=192):
        return lib.vaw_rk_stage(i, mt, c, u, ld, 2.5, x, xs, tab, row, rows, k, slots, a, nc, -0.1, xo, None, xn, 1e-5, 1e-4, part, cap, B, n, None)

    bad_slots = (C.c_int * 7)(0, 1, 2, 7, 4, 5, 6)
    for bad in (dict(i=7), dict(i=-1), dict(mt=4), dict(mt=-1), dict(x=None), dict(k=None), dict(slots=None), dict(a=None), dict(nc=8),
                dict(nc=-1), dict(c=None, u=p), dict(c=None, nc=0, xo=None), dict(tab=None), dict(row=7), dict(row=-1), dict(ld=191),
                dict(slots=bad_slots), dict(B=0), dict(n=0), dict(xo=None), dict(nc=0), dict(part=p, cap=3), dict(part=p, xn=p, cap=3),
                dict(part=p, xo=None, xn=p, cap=2), dict(part=4100, xo=None, xn=p, cap=3), dict(part=p, xo=None, xn=None, cap=3)):
        assert stage(**bad) == -1, bad
        assert b"rk_stage" in lib.vaw_last_error_string()

    def sumsq(u=p, v=None, a=p, b=None, part=p, cap=3, B=3, n=192):
        return lib.vaw_rk_scaled_sumsq(u, v, a, b, 1e-5, 1e-4, part, cap, B, n, None)

    for bad in (dict(u=None), dict(a=None), dict(part=None), dict(part=4100), dict(cap=2), dict(B=0), dict(n=0)):
        assert sumsq(**bad) == -1, bad
        assert b"rk_scaled_sumsq" in lib.vaw_last_error_string()
    for args in ((None, 3, p), (p, 3, None), (p, 0, p), (4100, 3, p), (p, 3, 4100)):
        assert lib.vaw_rk_sumsq_finish(*args, None) == -1, args
        assert b"rk_sumsq_finish" in lib.vaw_last_error_string()
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.rk_stage(0, "VELOCITY", x, None, 1.0, x, None, torch.zeros(7, 16), 0, torch.zeros(7, 2, 3, 8, 8), list(range(7)), (0.2,), -0.1, x_out=x)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.rk_scaled_sumsq(x, None, x, None, 1e-5, 1e-4, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.rk_sumsq_finish(torch.zeros(2, dtype=torch.float64), 2, torch.zeros(1, dtype=torch.float64))

"""Host side of the fused EDM / flow solver steps without a GPU: the per-grid tables against the scalars the loops compute
step by step, their cache, the `fused` keyword on CPU tensors, the C ABI's argument checks and Sampler's hip_graph refusals.

`composed_*` below restate the loops as they stood before the tables existed (tensor operations only); they are the
yardstick for `fused=False` here and are not imported by the package."""
import itertools

import numpy as np
import pytest
import torch

import abi_cases
import vaw_amd
from conftest import sampling_model
from sampler_cases import Standin, build, sampler_args
from vaw_amd import ops, samplers
from vaw_amd.gaussian_diffusion import ModelMeanType

DISCRETIZATIONS, SCHEDULES, SCALINGS = ("vp", "ve", "iddpm", "edm"), ("vp", "ve", "linear"), ("vp", "none")
PATH_TYPES = ("linear", "cosine", "linear_logsnr")


def edm_net(pred_type="EPSILON", model=None, device="cpu", **kw):
    return vaw_amd.EDMDenoiser(model or Standin(sampling_model), img_resolution=8, img_channels=3, pred_type=pred_type, label_dim=10,
                               **kw).to(device)


def flow(path_type, mean_type="VELOCITY"):
    return vaw_amd.FlowMatching(args=sampler_args("flow", dict(guidance_scale=1.0), path_type=path_type),
                                model_mean_type=ModelMeanType[mean_type])


# ---- the loops as tensor compositions ------------------------------------------------------------------------------------
def composed_edm_sample(net, latents, class_labels=None, randn_like=torch.randn_like, num_steps=18, sigma_min=None, sigma_max=None,
                        rho=7, solver="heun", discretization="edm", schedule="linear", scaling="none", epsilon_s=1e-3, alpha=1,
                        S_churn=0, S_min=0, S_max=float("inf"), S_noise=1, record=None, **model_kwargs):
    vp0 = lambda t: (np.e ** (0.5 * 19.9 * (t ** 2) + 0.1 * t) - 1) ** 0.5
    lo = {"vp": vp0(epsilon_s), "ve": 0.02, "iddpm": 0.002, "edm": 0.002}[discretization] if sigma_min is None else sigma_min
    hi = {"vp": vp0(1), "ve": 100, "iddpm": 81, "edm": 80}[discretization] if sigma_max is None else sigma_max
    lo, hi = max(lo, net.sigma_min), min(hi, net.sigma_max)
    bd = 2 * (np.log(lo ** 2 + 1) / epsilon_s - np.log(hi ** 2 + 1)) / (epsilon_s - 1)
    path = samplers._Path(schedule, scaling, bd, np.log(hi ** 2 + 1) - 0.5 * bd)
    levels = samplers._noise_levels(net, discretization, num_steps, lo, hi, rho, epsilon_s, latents.device)
    t_grid = path.sigma_inv(net.round_sigma(levels))
    t_grid = torch.cat([t_grid, torch.zeros_like(t_grid[:1])])
    x = latents.to(torch.float64) * (path.sigma(t_grid[0]) * path.s(t_grid[0]))

    def at(t):          # the scalars of one evaluation: EDMDenoiser.forward's and _Path.slope's
        sigma = path.sigma(t).to(torch.float32).reshape(-1, 1, 1, 1)
        c_in = 1 / (sigma ** 2 + 1).sqrt()
        step = (net.M - 1 - net.nearest_index(sigma).to(torch.float32)).flatten().repeat(latents.shape[0]).int()
        sg, dsg, sc = path.sigma(t), path.dsigma(t), path.s(t)
        return [path.s(t), sigma, c_in, c_in ** 2, sigma * c_in, dsg / sg + path.ds(t) / sc, dsg * sc / sg, step[0]], step

    for i in range(num_steps):
        t_cur, t_next = t_grid[i], t_grid[i + 1]
        sg_cur = path.sigma(t_cur)
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= sg_cur <= S_max else 0
        t_hat = path.sigma_inv(net.round_sigma(sg_cur + gamma * sg_cur))
        x_hat = (path.s(t_hat) / path.s(t_cur) * x
                 + (path.sigma(t_hat) ** 2 - sg_cur ** 2).clip(min=0).sqrt() * path.s(t_hat) * S_noise * randn_like(x))
        h = t_next - t_hat
        last = solver == "euler" or i == num_steps - 1
        if record is not None:
            hat, step_hat = at(t_hat)
            mid, step_mid = ([0.0] * 8, None) if last else at(t_hat + alpha * h)
            record.append(dict(row=[path.s(t_hat) / path.s(t_cur),
                                    (path.sigma(t_hat) ** 2 - sg_cur ** 2).clip(min=0).sqrt() * path.s(t_hat) * S_noise, *hat, h,
                                    alpha * h, 1 - 1 / (2 * alpha), 1 / (2 * alpha), *mid],
                               steps=(step_hat, step_mid), churn=gamma != 0,
                               t_mean=(float(step_hat.float().mean()), None if last else float(step_mid.float().mean()))))
        d_cur = path.slope(x_hat, t_hat, net(x_hat / path.s(t_hat), path.sigma(t_hat), class_labels, **model_kwargs).to(torch.float64))
        if last:
            x = x_hat + h * d_cur
            continue
        t_mid = t_hat + alpha * h
        x_mid = x_hat + alpha * h * d_cur
        d_mid = path.slope(x_mid, t_mid, net(x_mid / path.s(t_mid), path.sigma(t_mid), class_labels, **model_kwargs).to(torch.float64))
        x = x_hat + h * ((1 - 1 / (2 * alpha)) * d_cur + 1 / (2 * alpha) * d_mid)
    return x


def flow_scalars(fm, t_scalar, dt, batch, device):
    """What one evaluation of the flow loops computes that does not depend on x (the table row), and t as the network gets it."""
    like = torch.empty((batch, 1, 1, 1), device=device)
    t = fm.expand_t_like_x(t_scalar, like)
    a, s, da, ds = fm.interpolant(t)
    g2 = 2 * s * ds
    step = [0.0, 0.0, 0.0] if dt is None else [dt.to(torch.float32), torch.sqrt(torch.abs(dt)).to(torch.float32), (0.5 * dt).to(torch.float32)]
    row = [v[0] for v in (a, s, da, ds, g2, 0.5 * g2, s ** 2, a ** 2 + s ** 2, s * da - a * ds, torch.sqrt(g2))] + step + [t[0]]
    return row, t.view(batch)


def composed_flow_sde_sample(fm, model, noise, num_steps=50, solver="heun", randn_like=torch.randn_like, **model_kwargs):
    dev = noise.device
    grid = torch.cat([torch.linspace(1.0, 0.04, num_steps, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)])

    def drift_at(x, t_scalar):
        t, out = samplers._flow_eval(fm, model, x, t_scalar, model_kwargs)
        _, s, _, ds = fm.interpolant(t)
        g2 = 2 * s * ds
        v, score = samplers._flow_fields(fm, out, x, t)
        return v - 0.5 * g2 * score, g2

    x = noise
    for k in range(num_steps - 1):
        t0, t1 = grid[k], grid[k + 1]
        dt = t1 - t0
        f0, g2 = drift_at(x, t0)
        kick = torch.sqrt(g2) * randn_like(x) * torch.sqrt(torch.abs(dt))
        if solver == "euler":
            x = x + f0 * dt + kick
        else:
            f1, _ = drift_at(x + f0 * dt + kick, t1)
            x = x + 0.5 * (f0 + f1) * dt + kick
    f0, _ = drift_at(x, grid[-2])
    return x + f0 * (grid[-1] - grid[-2])


def composed_flow_ode_sample(fm, model, noise, num_steps=50, solver="heun", **model_kwargs):
    grid = torch.linspace(1.0, 0.0, num_steps, device=noise.device)
    v = lambda x, t_scalar: samplers._flow_fields(fm, samplers._flow_eval(fm, model, x, t_scalar, model_kwargs)[1], x,
                                                  fm.expand_t_like_x(t_scalar, x))[0]
    x = noise
    for k in range(num_steps - 1):
        t0, t1 = grid[k], grid[k + 1]
        dt = t1 - t0
        k1 = v(x, t0)
        x = x + dt * k1 if solver == "euler" else x + 0.5 * dt * (k1 + v(x + dt * k1, t1))
    return x


def bits(values, dtype):
    return torch.stack([(v.to(dtype) if torch.is_tensor(v) else torch.tensor(v, dtype=dtype)).reshape(()) for v in values])


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64 if a.element_size() == 8 else torch.int32),
                                                                     b.view(torch.int64 if b.element_size() == 8 else torch.int32))


# ---- tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discretization", DISCRETIZATIONS)
def test_edm_tables_hold_the_bits_of_the_scalars_the_loop_computes(discretization):
    net = edm_net()
    B, latents = 3, torch.zeros(3, 3, 8, 8)
    for schedule, scaling, num_steps, S_churn, solver in itertools.product(SCHEDULES, SCALINGS, (5, 18), (0, 40), ("heun", "euler")):
        if solver == "euler" and (num_steps, S_churn) != (5, 40):
            continue
        kw = dict(num_steps=num_steps, solver=solver, discretization=discretization, schedule=schedule, scaling=scaling, S_churn=S_churn,
                  S_min=0.05, S_max=50.0, S_noise=1.003)
        rec = []
        composed_edm_sample(net, latents, record=rec, **kw)
        lo, hi = samplers._edm_sigma_range(net, discretization, None, None, 1e-3)
        tab = samplers._edm_tables(net, latents.device, B, num_steps, lo, hi, 7, solver, discretization, schedule, scaling, 1e-3, 1,
                                   S_churn, 0.05, 50.0, 1.003)
        what = (discretization, schedule, scaling, num_steps, S_churn, solver)
        assert tab.coef.dtype == torch.float64 and tab.coef.shape == (num_steps, ops.EDM_COLS), what
        assert tab.steps.dtype == torch.int32 and tab.steps.shape == (2 * num_steps, 2 * B) and tab.steps.is_contiguous(), what
        assert bool(torch.isfinite(tab.coef).all()), what
        for i, r in enumerate(rec):
            assert same_bits(tab.coef[i, :22], bits(r["row"], torch.float64)), (what, i)
            assert tab.host[i] == tab.coef[i].tolist()
            assert tab.noise_on[i] == (float(r["row"][1]) != 0), (what, i)
            for half, step in enumerate(r["steps"]):
                if step is not None:
                    assert torch.equal(tab.steps[2 * i + half, :B], step) and torch.equal(tab.steps[2 * i + half, B:], step), (what, i)
                assert tab.t_mean[2 * i + half] == r["t_mean"][half], (what, i)
        if S_churn:          # S_min / S_max cut the churn off at both ends of this grid, and where it is on the step adds noise
            churn = [r["churn"] for r in rec]
            assert any(churn) and (num_steps == 5 or not all(churn)), what
            assert all(on for on, c in zip(tab.noise_on, churn) if c), what
        else:
            assert not any(tab.noise_on), what


@pytest.mark.parametrize("path_type", PATH_TYPES)
def test_flow_tables_hold_the_bits_of_the_scalars_the_loops_compute(path_type):
    fm, B, dev = flow(path_type), 3, torch.device("cpu")
    for kind, solver, num_steps in itertools.product(("sde", "ode"), ("heun", "euler"), (5, 18)):
        tab = samplers._flow_tables(fm, kind, solver, num_steps, B, dev)
        if kind == "sde":
            grid = torch.cat([torch.linspace(1.0, 0.04, num_steps, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)])
        else:
            grid = torch.linspace(1.0, 0.0, num_steps)
        evals = []
        for k in range(num_steps - 1):
            evals.append((grid[k], grid[k + 1] - grid[k]))
            if solver == "heun":
                evals.append((grid[k + 1], None))
        if kind == "sde":
            evals.append((grid[-2], grid[-1] - grid[-2]))
        assert tab.coef.dtype == torch.float32 and tab.coef.shape == (len(evals), ops.FLOW_COLS) and tab.coef.is_contiguous()
        assert tab.times.dtype == torch.float32 and tab.times.shape == (len(evals), 2 * B) and tab.times.is_contiguous()
        for e, (t_scalar, dt) in enumerate(evals):
            row, t = flow_scalars(fm, t_scalar, dt, B, dev)
            got, exp = tab.coef[e, :14], bits(row, torch.float32)
            nan = torch.isnan(exp)                        # sqrt(g2) where g2 rounds below zero (cosine path at t = 1)
            assert torch.equal(torch.isnan(got), nan) and same_bits(got[~nan], exp[~nan]), (path_type, kind, solver, num_steps, e)
            assert torch.equal(tab.times[e, :B], t) and torch.equal(tab.times[e, B:], t)
            assert tab.t_mean[e] == float(t.float().mean())


def test_tables_are_cached_per_grid_and_rebuilt_when_a_key_changes():
    net = edm_net()
    dev = torch.device("cpu")
    base = dict(device=dev, batch=3, num_steps=5, lo=0.002, hi=80.0, rho=7, solver="heun", discretization="edm", schedule="linear",
                scaling="none", epsilon_s=1e-3, alpha=1, S_churn=0, S_min=0, S_max=float("inf"), S_noise=1)
    first = samplers._edm_tables(net, **base)
    assert samplers._edm_tables(net, **base) is first and len(net._solver_tables) == 1
    changes = dict(batch=4, num_steps=6, lo=0.01, hi=50.0, rho=5, solver="euler", discretization="ve", schedule="ve", scaling="vp",
                   epsilon_s=2e-3, alpha=0.75, S_churn=10, S_min=0.1, S_max=10.0, S_noise=1.01)
    for n, (k, v) in enumerate(changes.items()):          # (the device is part of the key too: checked below)
        other = samplers._edm_tables(net, **{**base, k: v})
        assert other is not first and len(net._solver_tables) == n + 2, k
        assert samplers._edm_tables(net, **{**base, k: v}) is other
    assert all(str(dev) in key for key in net._solver_tables)
    assert samplers._edm_tables(edm_net(), **base) is not first          # per denoiser
    fm = flow("linear")
    fbase = dict(kind="sde", solver="heun", num_steps=5, batch=3, device=dev)
    first = samplers._flow_tables(fm, **fbase)
    assert samplers._flow_tables(fm, **fbase) is first
    for n, (k, v) in enumerate(dict(kind="ode", solver="euler", num_steps=6, batch=2).items()):
        assert samplers._flow_tables(fm, **{**fbase, k: v}) is not first and len(fm._solver_tables) == n + 2, k
    fm.path_type = "cosine"
    assert samplers._flow_tables(fm, **fbase) is not first
    assert all(str(dev) in key for key in fm._solver_tables)


# ---- the fused keyword on the CPU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,S_churn,pred_type", [("heun", 0, "EPSILON"), ("heun", 40, "VELOCITY"), ("euler", 40, "START_X")])
def test_edm_sample_unfused_is_the_composition_and_fused_needs_the_gpu(solver, S_churn, pred_type):
    net = edm_net(pred_type, vaw_amd.IntervalCFG(Standin(sampling_model), 10, 1.8, (100.0, 600.0), True))
    y = torch.tensor([1, 5, 9])
    kw = dict(class_labels=y, num_steps=6, solver=solver, S_churn=S_churn, S_min=0.05, S_max=50.0)
    outs = []
    for fn, extra in ((composed_edm_sample, {}), (vaw_amd.edm_sample, dict(fused=False)), (vaw_amd.edm_sample, {})):
        torch.manual_seed(3)
        outs.append(fn(net, torch.randn(3, 3, 8, 8), **kw, **extra))
        outs.append(torch.randn(2))          # the stream is where the composition leaves it
    assert outs[0].dtype == torch.float64 and bool(torch.isfinite(outs[0]).all())
    for k in (2, 4):
        assert torch.equal(outs[k], outs[0]) and outs[k].dtype == outs[0].dtype and torch.equal(outs[k + 1], outs[1])
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.edm_sample(net, torch.randn(3, 3, 8, 8), fused=True, **kw)
    with pytest.raises(ValueError, match="solver"):
        vaw_amd.edm_sample(net, torch.randn(3, 3, 8, 8), solver="dpm", fused=False)


@pytest.mark.parametrize("solver", ["heun", "euler"])
def test_flow_samplers_unfused_are_the_composition_and_fused_needs_the_gpu(solver):
    fm = flow("linear")
    model = vaw_amd.IntervalCFG(Standin(sampling_model), 10, 1.8, (0.2, 0.7), True)
    y = torch.tensor([1, 5, 9])
    for composed, fn in ((composed_flow_sde_sample, vaw_amd.flow_sde_sample), (composed_flow_ode_sample, vaw_amd.flow_ode_sample)):
        outs = []
        for f, extra in ((composed, {}), (fn, dict(fused=False)), (fn, {})):
            torch.manual_seed(4)
            outs.append(f(fm, model, torch.randn(3, 3, 8, 8), num_steps=6, solver=solver, y=y, **extra))
            outs.append(torch.randn(2))
        assert outs[0].dtype == torch.float32 and bool(torch.isfinite(outs[0]).all())
        for k in (2, 4):
            assert torch.equal(outs[k], outs[0]) and torch.equal(outs[k + 1], outs[1])
        with pytest.raises(ValueError, match="fused=True"):
            fn(fm, model, torch.randn(3, 3, 8, 8), num_steps=6, solver=solver, y=y, fused=True)
    with pytest.raises(NotImplementedError, match="dopri5"):
        vaw_amd.flow_ode_sample(fm, model, torch.randn(3, 3, 8, 8), solver="dopri5", y=y)
    for s in ("midpoint", "rk4"):          # still the tensor composition
        assert vaw_amd.flow_ode_sample(fm, model, torch.randn(3, 3, 8, 8), num_steps=4, solver=s, y=y).shape == (3, 3, 8, 8)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_solver_entry_points_have_argtypes_and_reject_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    for name, nargs in (("vaw_edm_input", 11), ("vaw_edm_step", 17), ("vaw_flow_step", 21)):
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        assert len(abi_cases.assert_bound_as_declared(lib, name)) == nargs
    assert (ops.EDM_COLS, ops.FLOW_COLS) == (24, 16)
    with open(f"{vaw_amd.__path__[0]}/../include/vaw_hip.h") as f:
        header = f.read()
    assert "#define VAW_EDM_COLS 24" in header and "#define VAW_FLOW_COLS 16" in header
    p = 4096          # never dereferenced: every call below fails its argument check

    def edm_in(x=p, nz=p, coef=p, row=1, rows=5, xh=p, mi=p, B=3, n=192):
        return lib.vaw_edm_input(x, nz, coef, row, rows, xh, mi, None, B, n, None)

    for bad in (dict(x=None), dict(coef=None), dict(xh=None), dict(mi=None), dict(B=0), dict(n=0), dict(row=5), dict(row=-1), dict(x=4100),
                dict(nz=4100)):
        assert edm_in(**bad) == -1, bad
        assert b"edm_input" in lib.vaw_last_error_string()

    def edm_st(kind=2, pred=0, c=p, u=p, ld=192, xh=p, dc=p, coef=p, row=1, rows=5, xo=p, mi=p, B=3, n=192):
        return lib.vaw_edm_step(kind, pred, c, u, ld, 2.5, xh, dc, coef, row, rows, xo, mi, None, B, n, None)

    for bad in (dict(kind=3), dict(kind=-1), dict(pred=3), dict(c=None), dict(xh=None), dict(coef=None), dict(ld=191), dict(row=5),
                dict(B=0), dict(n=0), dict(kind=2, dc=None), dict(kind=2, xo=None), dict(kind=0, xo=None), dict(kind=1, dc=None),
                dict(kind=1, mi=None), dict(xh=4100)):
        assert edm_st(**bad) == -1, bad
        assert b"edm_step" in lib.vaw_last_error_string()

    def flow_st(kind=2, sde=1, mt=2, c=p, u=p, ld=192, x=p, nz=None, xp=p, f0=p, kick=p, coef=p, r0=1, r1=2, rows=5, xo=p, B=3, n=192):
        return lib.vaw_flow_step(kind, sde, mt, c, u, ld, 2.5, x, nz, xp, f0, kick, coef, r0, r1, rows, xo, None, B, n, None)

    for bad in (dict(kind=3), dict(sde=2), dict(mt=4), dict(mt=-1), dict(c=None), dict(x=None), dict(coef=None), dict(xo=None), dict(ld=100),
                dict(r0=5), dict(r1=-1), dict(B=0), dict(n=0), dict(f0=None), dict(xp=None), dict(sde=0), dict(kind=1, nz=p, kick=None),
                dict(kind=1, f0=None)):
        assert flow_st(**bad) == -1, bad
        assert b"flow_step" in lib.vaw_last_error_string()
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.flow_step(0, False, "VELOCITY", x, None, 1.0, x, None, None, None, None, torch.zeros(2, 16), 0, 0, x)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.edm_input(x.double(), None, torch.zeros(2, 24, dtype=torch.float64), 0, x.double(), x)


# ---- Sampler --------------------------------------------------------------------------------------------------------------
def test_sampler_hip_graph_refusals():
    st = dict(guidance_scale=2.5, solver="heun", sample_steps=4)
    for kind, extra in (("edm", {}), ("flow", dict(path_type="linear", mean_type="VELOCITY"))):
        s = dict(st, **extra)
        for bad, match in ((dict(cpu_rng=True), "cpu_rng"), (dict(cpu_rng=False, parallel=True), "parallel")):
            args = sampler_args(kind, s, hip_graph=True, **bad)
            diff, model = build(kind, s, args)
            with pytest.raises(ValueError, match=match):
                vaw_amd.Sampler(args, "cpu", model, diff).sample(3, 3, 8, 10)
    for value in ("auto", False, None):          # eager, as without the attribute
        args = sampler_args("edm", st, hip_graph=value)
        torch.manual_seed(1)
        images, labels = vaw_amd.Sampler(args, "cpu", Standin(sampling_model), None).sample(3, 3, 8, 10)
        torch.manual_seed(1)
        ref, _ = vaw_amd.Sampler(sampler_args("edm", st), "cpu", Standin(sampling_model), None).sample(3, 3, 8, 10)
        assert (images[0] == ref[0]).all()

"""The linear multistep samplers (vaw_amd.dpm_sample: DPM-Solver++ 2M, 2M-SDE, exponential Adams-Bashforth) without a GPU: the
weights against quadrature, the order of convergence and the stationary variance on a Gaussian whose denoiser is known in
closed form, the composition against a loop written out in the textbook form, the per-grid tables and their cache, the
refusals, the C ABI's argument checks and Sampler's dispatch."""
import math

import pytest
import torch

import abi_cases
import vaw_amd
from conftest import sampling_model
from sampler_cases import Standin, build, sampler_args
from vaw_amd import ops, samplers

C2 = 0.25          # variance of the Gaussian data of the analytic denoiser


class Gaussian:
    """D(x; sigma) = c^2 / (c^2 + sigma^2) x, the exact denoiser of data ~ N(0, c^2 I): only the protocol dpm_sample's
    composition may use (the call, round_sigma, sigma_min, sigma_max).  Remembers the states it was called on."""
    sigma_min, sigma_max = 0.002, 80.0

    def __init__(self):
        self.seen = []

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)

    def __call__(self, x, sigma, class_labels=None):
        self.seen.append((x, sigma))
        return C2 / (C2 + sigma ** 2) * x


def edm_net(pred_type="EPSILON", model=None, **kw):
    return vaw_amd.EDMDenoiser(model or Standin(sampling_model), img_resolution=8, img_channels=3, pred_type=pred_type, label_dim=10, **kw)


def table(net, solver, num_steps=6, order=None, eta=0.0, s_noise=1.0, batch=3, discretization="edm"):
    lo, hi = samplers._edm_sigma_range(net, discretization, None, None, 1e-3)
    order = 3 if solver == "expab" and order is None else order
    return samplers._dpm_tables(net, torch.device("cpu"), batch, num_steps, lo, hi, 7, solver, order, discretization, 1e-3, eta, s_noise)


# ---- 1. the expab weights integrate what they say ------------------------------------------------------------------------------
def test_expab_weights_are_exact_on_polynomials_below_their_order():
    from scipy.integrate import quad
    lam, target = (0.3, -0.1, -0.35), 0.9
    for q in (1, 2, 3):
        b = [float(v) for v in samplers._expab_weights([torch.tensor(v, dtype=torch.float64) for v in lam[:q]],
                                                        torch.tensor(target, dtype=torch.float64))]
        assert len(b) == q
        for degree in range(q):
            exact, _ = quad(lambda tau: math.exp(-(target - tau)) * tau ** degree, lam[0], target, epsabs=1e-14, epsrel=1e-14)
            got = sum(bj * lj ** degree for bj, lj in zip(b, lam))
            print(f"expab q={q} degree={degree}: |sum - quad| = {abs(got - exact):.3e}")
            assert abs(got - exact) <= 1e-13, (q, degree, got, exact)


# ---- 2. order of convergence ------------------------------------------------------------------------------------------------
def gaussian_error(num_steps, **kw):
    """max |x - exact| at the last noise level before the final denoise step, from x(sigma_0) = sigma_0 * latents."""
    net = Gaussian()
    latents = torch.linspace(-2.0, 2.0, 16, dtype=torch.float64).reshape(1, 1, 4, 4)
    vaw_amd.dpm_sample(net, latents, num_steps=num_steps, fused=False, **kw)
    assert len(net.seen) == num_steps          # one evaluation per step
    x, sigma = net.seen[-1]
    sigma0 = net.seen[0][1]
    exact = latents * sigma0 * torch.sqrt((C2 + sigma ** 2) / (C2 + sigma0 ** 2))
    return float((x - exact).abs().max())


@pytest.mark.parametrize("kw,lo,hi", [(dict(solver="dpmpp2m"), 1.9, None), (dict(solver="expab", order=3), 2.8, None),
                                      (dict(solver="expab", order=1), 0.9, 1.1), (dict(solver="expab", order=2), 1.9, None),
                                      (dict(solver="expab"), 2.8, None)],
                         ids=["dpmpp2m", "expab3", "expab1", "expab2", "expab_default"])
def test_order_of_convergence_on_the_gaussian(kw, lo, hi):
    err = {n: gaussian_error(n, **kw) for n in (32, 64, 128)}
    rates = [math.log2(err[32] / err[64]), math.log2(err[64] / err[128])]
    print(f"{kw}: errors {err}, observed orders {rates[0]:.3f}, {rates[1]:.3f}")
    for r in rates:
        assert r >= lo and (hi is None or r <= hi), (kw, err, rates)


# ---- 3. the stochastic step ----------------------------------------------------------------------------------------------------
def test_sde_table_reaches_the_data_variance_and_eta_zero_is_dpmpp2m():
    net, steps = Gaussian(), 128
    tab = table(net, "dpmpp2m_sde", steps, eta=1.0)
    assert tab.noise_on == [True] * (steps - 1) + [False] and tab.steps is None
    sig, coef = tab.sigma.tolist(), tab.coef.tolist()
    cov = [[sig[0] ** 2, 0.0], [0.0, 0.0]]          # of (x, D_old), per element: x(sigma_0) = sigma_0 * N(0, 1), no history yet
    for i in range(steps - 1):
        a, b0, b1, b2, c = coef[i][:5]
        k = C2 / (C2 + sig[i] ** 2)
        assert b2 == 0.0 and (b1 == 0.0) == (i == 0)
        m = [[a + b0 * k, b1], [k, 0.0]]            # x' = a x + b0 (k x) + b1 D_old + c xi;  D_old' = k x
        mc = [[sum(m[r][j] * cov[j][s] for j in range(2)) for s in range(2)] for r in range(2)]
        cov = [[sum(mc[r][j] * m[s][j] for j in range(2)) for s in range(2)] for r in range(2)]
        cov[0][0] += c * c
    want = C2 + sig[steps - 1] ** 2
    print(f"variance at sigma_min {cov[0][0]:.6f} against {want:.6f}: off by {abs(cov[0][0] / want - 1):.4%}")
    assert abs(cov[0][0] / want - 1) <= 0.01
    for n in (6, steps):
        det, sde0 = table(net, "dpmpp2m", n), table(net, "dpmpp2m_sde", n, eta=0.0)
        assert det is not sde0 and torch.equal(sde0.coef, det.coef) and not any(sde0.noise_on)
        assert torch.equal(sde0.coef.view(torch.int64), det.coef.view(torch.int64))          # the same bits, signed zeros included


# ---- 4. the composition against the textbook loop ----------------------------------------------------------------------------
def textbook(net, latents, y, solver, num_steps, order=3, eta=1.0, s_noise=1.0, clip=False, record=None):
    """The three solvers as the papers write them (float64, no coefficient table): 2M in its midpoint form with the
    extrapolated denoised image, the SDE variant term by term, exponential Adams-Bashforth through Newton's divided
    differences of the denoised images."""
    lo, hi = samplers._edm_sigma_range(net, "edm", None, None, 1e-3)
    sig = net.round_sigma(samplers._noise_levels(net, "edm", num_steps, lo, hi, 7, 1e-3, latents.device))
    sig = torch.cat([sig, torch.zeros_like(sig[:1])])
    lam = lambda s: -torch.log(s)
    x = latents.to(torch.float64) * sig[0]
    old = []          # (lambda, denoised), newest first
    for i in range(num_steps):
        if record is not None:
            record.append(x)
        den = net(x, sig[i], y)
        if clip:
            den = den.clamp(-1, 1)
        den = den.to(torch.float64)
        s, s_next = sig[i], sig[i + 1]
        if i == num_steps - 1:
            x = den
            break
        h = lam(s_next) - lam(s)
        if solver == "dpmpp2m":
            d = den
            if old:
                r = (lam(s) - old[0][0]) / h
                d = (1 + 1 / (2 * r)) * den - (1 / (2 * r)) * old[0][1]
            x = (s_next / s) * x - torch.expm1(-h) * d
        elif solver == "dpmpp2m_sde":
            eta_h = eta * h
            x_new = s_next / s * torch.exp(-eta_h) * x + (-torch.expm1(-h - eta_h)) * den
            if old:
                r = (lam(s) - old[0][0]) / h
                x_new = x_new + 0.5 * (-torch.expm1(-h - eta_h)) * (1 / r) * (den - old[0][1])
            if eta > 0:
                x_new = x_new + torch.randn_like(x) * s_next * torch.sqrt(-torch.expm1(-2 * eta_h)) * s_noise
            x = x_new
        else:
            q = min(order, i + 1)
            I0 = -torch.expm1(-h)
            x_new = torch.exp(-h) * x + I0 * den
            if q >= 2:
                I1 = h - I0
                u1 = old[0][0] - lam(s)
                dd1 = (old[0][1] - den) / u1
                x_new = x_new + I1 * dd1
            if q >= 3:
                I2 = h ** 2 - 2 * I1
                dd2 = ((old[1][1] - old[0][1]) / (old[1][0] - old[0][0]) - dd1) / (old[1][0] - lam(s))
                x_new = x_new + (I2 - u1 * I1) * dd2
            x = x_new
        old = [(lam(s), den)] + old[:1]
    return x


class Recording(torch.nn.Module):
    """A denoiser that remembers the float64 states it is called on."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []
        self.sigma_min, self.sigma_max, self.round_sigma = net.sigma_min, net.sigma_max, net.round_sigma

    def forward(self, x, sigma, class_labels=None, **kw):
        self.seen.append(x)
        return self.net(x, sigma, class_labels, **kw)


@pytest.mark.parametrize("pred_type", ["EPSILON", "START_X", "VELOCITY"])
def test_composition_is_the_textbook_loop(pred_type):
    """Every state handed to the network, and the result, against the textbook forms at rtol 1e-12: the coefficient form
    differs from them by a few float64 roundings of its O(1) weights times the terms they multiply.  The difference is
    therefore taken relative to the largest magnitude of the state (max |a - b| <= 1e-12 max |b| per state): relative to the
    element itself no bound holds between two orders of a sum whose terms cancel (measured: an element of value 3.5e-4 formed
    from O(1) terms differs by 3.8e-15, 1.07e-11 of itself; 1 of 576 elements of that state exceeds 1e-12 that way).
    Largest relative difference seen over the three prediction types and five settings: 9.7e-16 (EPSILON 9.7e-16, START_X
    8.0e-16, VELOCITY 6.0e-16).  Also: fused=None on CPU tensors is fused=False bit for bit, generator offset included."""
    cfg = vaw_amd.IntervalCFG(Standin(sampling_model), 10, 1.8, (100.0, 600.0), True)
    net = edm_net(pred_type, cfg)
    y = torch.tensor([1, 5, 9])
    worst = elementwise = 0.0
    for kw in (dict(solver="dpmpp2m"), dict(solver="dpmpp2m_sde", eta=0.7, s_noise=1.003), dict(solver="expab", order=3),
               dict(solver="expab", order=2), dict(solver="dpmpp2m", clip=True)):
        clip = kw.pop("clip", False)
        torch.manual_seed(5)
        states = []
        ref = textbook(net, torch.randn(3, 3, 8, 8), y, num_steps=6, clip=clip, record=states, **kw)
        ref_next = torch.randn(2)
        outs = {}
        for fused in (False, None):
            torch.manual_seed(5)
            rec = Recording(net)
            got = vaw_amd.dpm_sample(rec, torch.randn(3, 3, 8, 8), class_labels=y, num_steps=6, fused=fused, clip_denoised=clip, **kw)
            assert torch.equal(torch.randn(2), ref_next), "the generator was left at another offset"
            assert got.dtype == torch.float64 and len(rec.seen) == len(states) == 6
            outs[fused] = (got, rec.seen)
        got, seen = outs[False]
        assert torch.equal(outs[None][0], got) and all(torch.equal(a, b) for a, b in zip(outs[None][1], seen))
        for k, (a, b) in enumerate(zip(seen + [got], states + [ref])):
            rel = float((a - b).abs().max() / b.abs().max())
            worst, elementwise = max(worst, rel), max(elementwise, float(((a - b).abs() / b.abs()).max()))
            assert rel <= 1e-12, (kw, k, rel)
        assert bool(torch.isfinite(got).all()) and (not clip or float(got.abs().max()) <= 1.0)
        print(f"{pred_type} {kw} clip={clip}: largest relative difference {worst:.3e} (elementwise, to the element itself: {elementwise:.3e})")
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.dpm_sample(net, torch.randn(3, 3, 8, 8), class_labels=y, num_steps=6, fused=True)


# ---- 5. tables -------------------------------------------------------------------------------------------------------------------
def test_tables_hold_the_networks_chain_indices_the_node_counts_and_are_cached():
    B, seen = 3, []

    def capture(x, t, **kw):
        seen.append(t)
        return x

    net = edm_net(model=Standin(capture))
    for solver, order, eta, steps in (("dpmpp2m", None, 0.0, 6), ("dpmpp2m_sde", None, 1.0, 6), ("dpmpp2m_sde", None, 0.0, 5),
                                      ("expab", 3, 0.0, 6), ("expab", 2, 0.0, 6), ("expab", 1, 0.0, 4)):
        tab = table(net, solver, steps, order=order, eta=eta, batch=B)
        assert tab.coef.dtype == torch.float64 and tab.coef.shape == (steps, ops.DPM_COLS) and tab.coef.is_contiguous()
        assert tab.steps.dtype == torch.int32 and tab.steps.shape == (steps, 2 * B) and tab.steps.is_contiguous()
        assert bool(torch.isfinite(tab.coef).all()) and float(tab.sigma[-1]) == 0.0 and tab.sigma.shape == (steps + 1,)
        assert tab.coef[-1, :5].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]          # the last step returns the denoised image
        for i in range(steps):
            del seen[:]
            net(torch.zeros(B, 3, 8, 8), tab.sigma[i])
            assert torch.equal(tab.steps[i, :B], seen[0]) and torch.equal(tab.steps[i, B:], seen[0]), (solver, i)
            assert tab.t_mean[i] == float(seen[0].float().mean())
            sigma = tab.sigma[i].to(torch.float32)
            c_in = 1 / (sigma ** 2 + 1).sqrt()
            c_next = 1 / (tab.sigma[i + 1].to(torch.float32) ** 2 + 1).sqrt() if i < steps - 1 else torch.zeros(())
            want = torch.stack([sigma, c_in, c_in ** 2, sigma * c_in, c_next]).to(torch.float64)
            assert torch.equal(tab.coef[i, 5:10], want), (solver, i)
            assert tab.coef[i, 10:].tolist() == [0.0, 0.0]
        q = order if solver == "expab" else 2
        assert tab.nodes == [min(q, i + 1) for i in range(steps - 1)] + [1], (solver, tab.nodes)
        assert tab.noise_on == [solver == "dpmpp2m_sde" and eta > 0] * (steps - 1) + [False]
        for i in range(steps):          # the weights beyond a step's nodes are zero: the kernel is not handed those images
            assert all(v == 0.0 for v in tab.coef[i, 1 + tab.nodes[i]:4].tolist())
    net = edm_net()
    first = table(net, "expab", order=3)
    assert table(net, "expab", order=3) is first and len(net._solver_tables) == 1
    for n, kw in enumerate((dict(order=2), dict(batch=4), dict(num_steps=7), dict(discretization="ve"))):
        assert table(net, "expab", **{"order": 3, **kw}) is not first and len(net._solver_tables) == n + 2
    sde = table(net, "dpmpp2m_sde", eta=1.0)
    assert table(net, "dpmpp2m_sde", eta=1.0) is sde
    assert table(net, "dpmpp2m_sde", eta=0.5) is not sde and table(net, "dpmpp2m_sde", eta=1.0, s_noise=1.1) is not sde
    assert all(str(torch.device("cpu")) in key for key in net._solver_tables)
    # dpm_sample goes through the same cache: a second call builds nothing
    z = torch.zeros(3, 3, 8, 8)
    vaw_amd.dpm_sample(net, z, num_steps=6, solver="expab", fused=False)
    count = len(net._solver_tables)
    vaw_amd.dpm_sample(net, z, num_steps=6, solver="expab", order=3, fused=False)
    assert len(net._solver_tables) == count
    vaw_amd.dpm_sample(net, z, num_steps=6, solver="dpmpp2m_sde", eta=0.25, fused=False)
    assert len(net._solver_tables) == count + 1


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    net, z = edm_net(), torch.randn(2, 3, 8, 8)
    for kw, match in ((dict(solver="heun"), "solver"), (dict(solver="dpm"), "solver"), (dict(solver="expab", order=0), "order"),
                      (dict(solver="expab", order=4), "order"), (dict(solver="dpmpp2m", order=2), "order"),
                      (dict(solver="dpmpp2m_sde", order=2), "order"), (dict(solver="dpmpp2m_sde", eta=-0.1), "eta"),
                      (dict(solver="dpmpp2m_sde", s_noise=-1.0), "s_noise"), (dict(solver="dpmpp2m", eta=-1.0), "eta"),
                      (dict(num_steps=1), "num_steps"), (dict(fused=True), "fused=True")):
        with pytest.raises(ValueError, match=match):
            vaw_amd.dpm_sample(net, z, **{"num_steps": 6, **kw})
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.dpm_sample(edm_net("SCORE"), z, num_steps=6, fused=True)
    # a range so narrow that the chain has one level in it: every snapped level coincides with the next
    for solver in samplers.DPM_SOLVERS:
        with pytest.raises(ValueError, match="step 0"):
            vaw_amd.dpm_sample(net, z, num_steps=6, solver=solver, sigma_min=1.0, sigma_max=1.001, fused=False)
    assert not net.__dict__.get("_solver_tables")          # a refused grid is not cached
    for solver in samplers.DPM_SOLVERS + ("dpm",):          # edm_sample still knows euler and heun only
        with pytest.raises(ValueError, match="solver"):
            vaw_amd.edm_sample(net, z, solver=solver, fused=False)


# ---- 7. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_check_their_arguments_before_any_launch():
    import re

    lib = vaw_amd.lib()
    with open(f"{vaw_amd.__path__[0]}/../include/vaw_hip.h") as f:
        header = f.read()
    for name, nargs in (("vaw_dpm_input", 9), ("vaw_dpm_step", 20)):
        assert re.search(rf"\bint {name}\(", header) and name in vaw_amd.exported_symbols() and hasattr(lib, name)
        assert len(abi_cases.assert_bound_as_declared(lib, name)) == nargs
    assert f"#define VAW_DPM_COLS {ops.DPM_COLS}\n" in header
    p = 4096          # never dereferenced: every call below fails its argument check

    def dpm_in(x=p, coef=p, row=1, rows=5, mi=p, dup=None, B=3, n=192):
        return lib.vaw_dpm_input(x, coef, row, rows, mi, dup, B, n, None)

    for bad in (dict(x=None), dict(coef=None), dict(mi=None), dict(B=0), dict(n=0), dict(row=5), dict(row=-1), dict(x=4100), dict(coef=4100)):
        assert dpm_in(**bad) == -1, bad
        assert b"dpm_input" in lib.vaw_last_error_string()

    def dpm_st(pred=0, c=p, u=p, ld=192, x=p, d1=p, d2=p, nz=p, coef=p, row=1, rows=5, xo=p, d0=p, mi=p, dup=p, B=3, n=192):
        return lib.vaw_dpm_step(pred, 1, c, u, ld, 2.5, x, d1, d2, nz, coef, row, rows, xo, d0, mi, dup, B, n, None)

    for bad in (dict(pred=3), dict(pred=-1), dict(c=None), dict(x=None), dict(coef=None), dict(xo=None), dict(d0=None), dict(ld=191),
                dict(row=5), dict(row=-1), dict(B=0), dict(n=0), dict(x=4100), dict(nz=4100), dict(xo=4100), dict(coef=4100),
                dict(d1=None), dict(mi=None)):          # (the last two: d2 without d1, model_in_dup without model_in)
        assert dpm_st(**bad) == -1, bad
        assert b"dpm_step" in lib.vaw_last_error_string()
    x = torch.zeros(2, 3, 8, 8)
    coef = torch.zeros(2, ops.DPM_COLS, dtype=torch.float64)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.dpm_input(x.double(), coef, 0, x)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.dpm_step("EPSILON", False, x, None, 1.0, x.double(), None, None, None, coef, 0, x.double(), x)


# ---- 8. Sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", samplers.DPM_SOLVERS)
def test_sampler_dispatches_the_multistep_solvers(solver):
    st = dict(guidance_scale=2.5, solver=solver, sample_steps=5)
    runs = []
    for _ in range(2):
        torch.manual_seed(1)
        images, labels = vaw_amd.Sampler(sampler_args("edm", st), "cpu", Standin(sampling_model), None).sample(6, 3, 8, 10)
        assert len(images) == len(labels) == 2
        assert all(b.dtype.name == "uint8" and b.shape == (3, 8, 8, 3) for b in images)
        runs.append((images, labels))
    for b in range(2):
        assert (runs[0][0][b] == runs[1][0][b]).all() and (runs[0][1][b] == runs[1][1][b]).all()
    assert (runs[0][0][0] != runs[0][0][1]).any()
    # the optional fields reach dpm_sample
    extra = {"dpmpp2m": dict(clip_denoised=True), "dpmpp2m_sde": dict(eta=0.3, s_noise=1.1), "expab": dict(order=1)}[solver]
    torch.manual_seed(1)
    other, _ = vaw_amd.Sampler(sampler_args("edm", st, **extra), "cpu", Standin(sampling_model), None).sample(3, 3, 8, 10)
    assert other[0].shape == (3, 8, 8, 3) and (solver == "dpmpp2m" or (other[0] != runs[0][0][0]).any())
    with pytest.raises(ValueError, match="order"):
        vaw_amd.Sampler(sampler_args("edm", st, order=4), "cpu", Standin(sampling_model), None).sample(3, 3, 8, 10)
    for bad, match in ((dict(cpu_rng=True), "cpu_rng"), (dict(cpu_rng=False, parallel=True), "parallel")):
        args = sampler_args("edm", st, hip_graph=True, **bad)
        _, model = build("edm", st, args)
        with pytest.raises(ValueError, match=match):
            vaw_amd.Sampler(args, "cpu", model, None).sample(3, 3, 8, 10)

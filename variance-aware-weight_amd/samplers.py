"""Samplers on the other side of training that reuse the HIP denoisers' forward kernels:

  * `EDMDenoiser` + `edm_sample`: the Karras et al. (EDM) deterministic / stochastic Euler-Heun sampler over a DDPM-trained
    denoiser -- behaviour of the reference's tools/cfg_edm.py (`Net` :15-108, `ablation_sampler` :111-210) as driven by
    tools/sampler.py:160-196 (`--solver euler|heun`, `--discretization`, `--schedule`, `--scaling`);
  * `dpm_sample`: linear multistep solvers in the data-prediction form over the same denoiser and noise levels (DPM-Solver++ 2M,
    its SDE variant, exponential Adams-Bashforth up to order 3; no counterpart in the reference): one network evaluation per
    step, the update x' = a x + b0 D0 + b1 D1 + b2 D2 + c noise from a per-grid table (`_dpm_tables`), one kernel per step
    (vaw_dpm_step).
  * `flow_sde_sample`, `flow_ode_sample`: the FlowMatching samplers of tools/gaussian_diffusion.py:1343-1417.  The reference's
    ODE sampler integrates with torchdiffeq (adaptive dopri5 by default), which is not available here: the fixed-grid
    solvers euler / midpoint / heun / rk4 are provided on the same time grid, and the adaptive integrator is provided under
    a name of its own, `solver="rk45"`: the same Dormand-Prince 5(4) pair with first-same-as-last stage reuse, driven by the
    step controller of scipy.integrate.solve_ivp(method="RK45") and pinned against it (tests/golden/rk45.npz).  It clips
    its last step to land on t = 0 where torchdiffeq steps past the end and interpolates back, and torchdiffeq's controller
    differs in details nothing here can check, so `dopri5` itself stays refused: step-for-step equality with torchdiffeq
    is unpinned and not claimed.  The SDE sampler is self-contained in the reference and pinned by tests/golden/samplers.pt.
  * `flow_log_likelihood`: the same ODE run from data to noise together with the integral of its divergence, i.e. the
    per-sample log-likelihood of a flow model (no counterpart in the reference): Hutchinson probes, one vector-Jacobian
    product per evaluation under `model.input_grad_only()`, and one kernel per stage (vaw_flow_logp_stage).

The denoiser call is the hot part and runs on the HIP kernels.  On the GPU the update around it is fused too (`fused=None`):
everything of a step that does not depend on x is computed once per grid into a device table, cached on the denoiser / flow
object (`_edm_tables`, `_flow_tables`), and the Euler / Heun steps are single streaming kernels (vaw_edm_input, vaw_edm_step,
vaw_flow_step; float64 for EDM, as in the reference) that read the table by row, fold the classifier-free guidance
combination in and write the next network input: bitwise the tensor composition (`fused=False`), with no host
synchronisation once the tables are cached, so a whole call can be captured into a graph.  The adaptive solver is the
exception: the host decides every step from one 8-byte read-back of the error norm (vaw_rk_stage, vaw_rk_scaled_sumsq)."""

import contextlib
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .gaussian_diffusion import ModelMeanType

__all__ = ["EDMDenoiser", "edm_sample", "dpm_sample", "flow_sde_sample", "flow_ode_sample", "flow_log_likelihood"]


def _unwrap(out):
    return out[0] if isinstance(out, tuple) else out


# ---------------------------------------------------------------------------------------------------------------------
# EDM
# ---------------------------------------------------------------------------------------------------------------------
class EDMDenoiser(torch.nn.Module):
    """D(x; sigma) for a network trained on the discrete DDPM chain (iDDPM preconditioning of the EDM paper): the noise level
    is snapped to the chain's sigma table u_j (u_M = 0, u_{j-1} = sqrt((u_j^2 + 1) / max(abar_{j-1}/abar_j, C_1) - 1)), the
    network sees x / sqrt(sigma^2 + 1) and the chain index M - 1 - j, and its eps / x0 / v output is mapped to x0."""

    def __init__(self, model, img_resolution, img_channels, pred_type="EPSILON", label_dim=0, amp=False, C_1=0.001, C_2=0.008,
                 M=1000, noise_schedule="linear", lambda_max=10.0, lambda_min=-10.0):
        super().__init__()
        self.model, self.img_resolution, self.img_channels, self.label_dim = model, img_resolution, img_channels, label_dim
        self.pred_type, self.M, self.C_1, self.C_2 = pred_type, M, C_1, C_2
        self.noise_schedule, self.lambda_max, self.lambda_min = noise_schedule, lambda_max, lambda_min
        self.amp = amp
        u = torch.zeros(M + 1)                               # float32, as the chain's table is kept by the reference
        for j in range(M, 0, -1):
            hi, lo = self._alpha_bar(j - 1), self._alpha_bar(j)
            ratio = (hi / lo).clip(min=C_1)
            if not torch.is_tensor(ratio):
                ratio = float(ratio)                         # a float64 numpy scalar acts as a weak (python) scalar on float32
            u[j - 1] = ((u[j] ** 2 + 1) / ratio - 1).sqrt()
        self.register_buffer("u", u)
        self.sigma_min, self.sigma_max = float(u[M - 1]), float(u[0])

    def _alpha_bar(self, j):
        """abar of chain position j (0 = pure noise end of the table) in the arithmetic each schedule is defined in: float32
        0-dim tensors for the closed forms, float64 numpy for the tabulated linear-beta product."""
        M = self.M
        jt = torch.as_tensor(j)
        if self.noise_schedule == "cosine":
            return (0.5 * np.pi * jt / M / (self.C_2 + 1)).sin() ** 2
        if self.noise_schedule == "linear":
            if not hasattr(self, "_acp"):
                self._acp = np.cumprod(1.0 - np.linspace(0.0001, 0.02, M + 1, dtype=np.float64), axis=0)
            return self._acp[M - j]
        if self.noise_schedule == "linear_logsnr":
            t = (M - jt) / M
            return torch.sigmoid(self.lambda_max + t * (self.lambda_min - self.lambda_max))
        raise NotImplementedError(f"unknown path type: {self.noise_schedule}")

    def nearest_index(self, sigma):
        sigma = torch.as_tensor(sigma)
        flat = sigma.to(self.u.device, torch.float32).reshape(-1, 1)
        return (flat - self.u.reshape(1, -1)).abs().argmin(1).reshape(sigma.shape).to(sigma.device)

    def round_sigma(self, sigma, return_index=False):
        sigma = torch.as_tensor(sigma)
        idx = self.nearest_index(sigma)
        if return_index:
            return idx
        return self.u[idx.flatten().to(self.u.device)].to(sigma.dtype).reshape(sigma.shape).to(sigma.device)

    def forward(self, x, sigma, class_labels=None, **model_kwargs):
        x = x.to(torch.float32)
        sigma = sigma.to(torch.float32).reshape(-1, 1, 1, 1)
        c_in = 1 / (sigma ** 2 + 1).sqrt()
        step = (self.M - 1 - self.nearest_index(sigma).to(torch.float32)).flatten().repeat(x.shape[0]).int()
        out = _unwrap(self.model((c_in * x), step, y=class_labels, **model_kwargs))[:, : self.img_channels].to(torch.float32)
        if self.pred_type == "EPSILON":
            return x - sigma * out
        if self.pred_type == "START_X":
            return out
        if self.pred_type == "VELOCITY":
            return c_in ** 2 * x - sigma * c_in * out
        raise ValueError(f"Unsupported pred_type: {self.pred_type}")


class _Path:
    """Noise-level path sigma(t) with its derivative / inverse, and the signal scaling s(t), of the EDM sampler family."""

    def __init__(self, schedule, scaling, beta_d, beta_min):
        if schedule not in ("vp", "ve", "linear") or scaling not in ("vp", "none"):
            raise ValueError(f"schedule {schedule!r} / scaling {scaling!r}")
        self.schedule, self.scaling, self.bd, self.bm = schedule, scaling, beta_d, beta_min

    def sigma(self, t):
        if self.schedule == "vp":
            return (np.e ** (0.5 * self.bd * (t ** 2) + self.bm * t) - 1) ** 0.5
        return t.sqrt() if self.schedule == "ve" else t

    def dsigma(self, t):
        if self.schedule == "vp":
            sg = self.sigma(t)
            return 0.5 * (self.bm + self.bd * t) * (sg + 1 / sg)
        return 0.5 / t.sqrt() if self.schedule == "ve" else 1

    def sigma_inv(self, sg):
        if self.schedule == "vp":
            return ((self.bm ** 2 + 2 * self.bd * (sg ** 2 + 1).log()).sqrt() - self.bm) / self.bd
        return sg ** 2 if self.schedule == "ve" else sg

    def s(self, t):
        return 1 / (1 + self.sigma(t) ** 2).sqrt() if self.scaling == "vp" else 1

    def ds(self, t):
        return -self.sigma(t) * self.dsigma(t) * (self.s(t) ** 3) if self.scaling == "vp" else 0

    def slope(self, x, t, denoised):
        """dx/dt of the probability-flow ODE at (x, t)."""
        sg, dsg, sc = self.sigma(t), self.dsigma(t), self.s(t)
        return (dsg / sg + self.ds(t) / sc) * x - dsg * sc / sg * denoised


def _noise_levels(net, discretization, num_steps, sigma_min, sigma_max, rho, epsilon_s, device):
    """The decreasing sigma grid of `discretization` (float64)."""
    i = torch.arange(num_steps, dtype=torch.float64, device=device)
    frac = i / (num_steps - 1)
    if discretization == "edm":
        return (sigma_max ** (1 / rho) + frac * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    if discretization == "ve":
        return ((sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** frac)).sqrt()
    if discretization == "vp":
        bd = 2 * (np.log(sigma_min ** 2 + 1) / epsilon_s - np.log(sigma_max ** 2 + 1)) / (epsilon_s - 1)
        bm = np.log(sigma_max ** 2 + 1) - 0.5 * bd
        t = 1 + frac * (epsilon_s - 1)
        return (np.e ** (0.5 * bd * (t ** 2) + bm * t) - 1) ** 0.5
    if discretization == "iddpm":
        M, C_1, C_2 = net.M, net.C_1, net.C_2
        abar = lambda k: (0.5 * np.pi * k / M / (C_2 + 1)).sin() ** 2          # always the cosine chain; float32 (k: int64 tensor)
        u = torch.zeros(M + 1, dtype=torch.float64, device=device)
        for k in torch.arange(M, 0, -1, device=device):
            u[k - 1] = ((u[k] ** 2 + 1) / (abar(k - 1) / abar(k)).clip(min=C_1) - 1).sqrt()
        u = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
        return u[((len(u) - 1) / (num_steps - 1) * i).round().to(torch.int64)]
    raise ValueError(f"discretization {discretization!r}")


def _want_fused(fused, x, what, unsupported):
    """Resolve the `fused` keyword of the samplers: None = fused where it is supported (GPU tensors), False = the tensor
    composition, True = fused or an error."""
    if fused is False:
        return False
    if not x.is_cuda:
        unsupported = "tensors on the CPU (the fused steps are HIP kernels)"
    if unsupported is None:
        return True
    if fused:
        raise ValueError(f"{what}: fused=True is not supported for {unsupported}")
    return False


def _row(values, dtype, device, cols):
    """A table row from the scalars the loops compute (0-dim / one-element tensors or Python numbers), widened exactly."""
    vals = [(v.to(dtype) if torch.is_tensor(v) else torch.tensor(v, dtype=dtype, device=device)).reshape(()) for v in values]
    return torch.stack(vals + [torch.zeros((), dtype=dtype, device=device)] * (cols - len(vals)))


def _guidance(model, y, t_mean, model_kwargs):
    """What the fused loops need to know of an IntervalCFG model: the wrapper (None for any other model), which evaluations
    are guided (the host-side predicate on the mean timestep of each, None = not evaluated), the scale, the stacked labels."""
    cfg = model if hasattr(model, "guided_halves") else None
    can = cfg is not None and cfg.class_cond and y is not None
    guided = [can and tm is not None and cfg.guidance_active(tm) for tm in t_mean]
    y2 = None
    if any(guided):
        y2 = {**model_kwargs, "y": torch.cat((y, y.new_full(y.shape, cfg.null_label)))}
    return cfg, guided, (cfg.guidance_scale if cfg is not None else 1.0), y2


def _evaluate(model, cfg, guided, stacked_kwargs, buf, n, t_rows, e, channels, model_kwargs):
    """One network evaluation of a fused loop on the input buffer `buf` ([2n, ...] when any evaluation of the grid is
    guided): the (conditional, unconditional or None) x-shaped float32 views of its output, left where the network wrote it."""
    if guided[e]:
        out = cfg.model(buf, t_rows[e], **stacked_kwargs)
    elif cfg is not None:
        out = cfg.unguided(buf[:n], t_rows[e, :n], **model_kwargs)
    else:
        out = model(buf[:n], t_rows[e, :n], **model_kwargs)
    out = _unwrap(out)
    if channels is not None:
        out = out[:, :channels]
    if out.dtype != torch.float32:
        out = out.to(torch.float32)
    return (out[:n], out[n:]) if guided[e] else (out, None)


def _edm_sigma_range(net, discretization, sigma_min, sigma_max, epsilon_s):
    vp0 = lambda t: (np.e ** (0.5 * 19.9 * (t ** 2) + 0.1 * t) - 1) ** 0.5
    lo = {"vp": vp0(epsilon_s), "ve": 0.02, "iddpm": 0.002, "edm": 0.002}[discretization] if sigma_min is None else sigma_min
    hi = {"vp": vp0(1), "ve": 100, "iddpm": 81, "edm": 80}[discretization] if sigma_max is None else sigma_max
    return max(lo, net.sigma_min), min(hi, net.sigma_max)


def _edm_time_grid(net, device, num_steps, lo, hi, rho, discretization, schedule, scaling, epsilon_s):
    bd = 2 * (np.log(lo ** 2 + 1) / epsilon_s - np.log(hi ** 2 + 1)) / (epsilon_s - 1)
    path = _Path(schedule, scaling, bd, np.log(hi ** 2 + 1) - 0.5 * bd)
    levels = _noise_levels(net, discretization, num_steps, lo, hi, rho, epsilon_s, device)
    t_grid = path.sigma_inv(net.round_sigma(levels))
    return path, torch.cat([t_grid, torch.zeros_like(t_grid[:1])])


def _edm_tables(net, device, batch, num_steps, lo, hi, rho, solver, discretization, schedule, scaling, epsilon_s, alpha, S_churn,
                S_min, S_max, S_noise):
    """Everything of edm_sample's loop that does not depend on x, computed once per grid with the loop's own expressions on
    `device` (so each entry has the bits of the scalar the composition computes at that step) and cached on the denoiser:
      coef    [num_steps, ops.EDM_COLS] float64 on the device: the rows vaw_edm_input / vaw_edm_step read (include/vaw_hip.h)
      steps   [2 * num_steps, 2 * batch] int32 on the device: the chain index handed to the network at t_hat (row 2i) and
              t_mid (row 2i + 1); a guided call takes a whole row, any other its first half
      scale0  sigma(t_0) * s(t_0), as the loop forms it
      noise_on, t_mean   host lists: does step i add noise, and the mean timestep as the network sees it at each evaluation
              (None where the solver does not evaluate) -- the argument of the guidance predicate
      host    the rows of coef on the host (one read-back together with t_mean)."""
    key = (solver, num_steps, discretization, schedule, scaling, float(lo), float(hi), rho, epsilon_s, alpha, S_churn, S_min, S_max,
           S_noise, int(batch), str(device))
    cache = net.__dict__.setdefault("_solver_tables", {})
    if key in cache:
        return cache[key]
    path, t_grid = _edm_time_grid(net, device, num_steps, lo, hi, rho, discretization, schedule, scaling, epsilon_s)

    def evaluation(t):
        sigma = path.sigma(t).to(torch.float32).reshape(-1, 1, 1, 1)          # EDMDenoiser.forward
        c_in = 1 / (sigma ** 2 + 1).sqrt()
        step = (net.M - 1 - net.nearest_index(sigma).to(torch.float32)).flatten()
        sg, dsg, sc = path.sigma(t), path.dsigma(t), path.s(t)                  # _Path.slope
        return [sc, sigma, c_in, c_in ** 2, sigma * c_in, dsg / sg + path.ds(t) / sc, dsg * sc / sg, step], step

    rows, steps, t_mean = [], [], []
    none = torch.zeros(1, device=device)
    for i in range(num_steps):
        t_cur, t_next = t_grid[i], t_grid[i + 1]
        sg_cur = path.sigma(t_cur)
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= sg_cur <= S_max else 0
        t_hat = path.sigma_inv(net.round_sigma(sg_cur + gamma * sg_cur))
        h = t_next - t_hat
        heun = solver == "heun" and i < num_steps - 1
        hat, step_hat = evaluation(t_hat)
        mid, step_mid = evaluation(t_hat + alpha * h) if heun else ([0.0] * 8, none)
        rows.append(_row([path.s(t_hat) / path.s(t_cur),
                          (path.sigma(t_hat) ** 2 - sg_cur ** 2).clip(min=0).sqrt() * path.s(t_hat) * S_noise, *hat, h, alpha * h,
                          1 - 1 / (2 * alpha), 1 / (2 * alpha), *mid], torch.float64, device, ops.EDM_COLS))
        for step, used in ((step_hat, True), (step_mid, heun)):
            steps.append(step.repeat(2 * batch).int())
            t_mean.append(steps[-1][:batch].float().mean() if used else none[0])          # IntervalCFG.forward's read-back
    coef = torch.stack(rows).contiguous()
    host = torch.cat([coef.flatten(), torch.stack(t_mean).to(torch.float64)]).tolist()
    n = coef.numel()
    used = [solver == "heun" and (e // 2) < num_steps - 1 if e % 2 else True for e in range(2 * num_steps)]
    tab = SimpleNamespace(coef=coef, steps=torch.stack(steps).contiguous(), scale0=path.sigma(t_grid[0]) * path.s(t_grid[0]),
                          host=[host[i * ops.EDM_COLS:(i + 1) * ops.EDM_COLS] for i in range(num_steps)],
                          t_mean=[tm if u else None for tm, u in zip(host[n:], used)], solver=solver, num_steps=num_steps)
    tab.noise_on = [r[1] != 0 for r in tab.host]
    cache[key] = tab
    return tab


def _edm_sample_fused(net, latents, class_labels, randn_like, tab, model_kwargs):
    """edm_sample's loop on the fused kernels: per step the noise draw, vaw_edm_input, the network, vaw_edm_step (and for a
    Heun step the network and vaw_edm_step again).  No host synchronisation."""
    n, shape = latents.shape[0], tuple(latents.shape)
    kwargs = {**model_kwargs, "y": class_labels}
    cfg, guided, scale, stacked = _guidance(net.model, class_labels, tab.t_mean, kwargs)
    if stacked is not None and class_labels.shape[0] != n:
        raise AssertionError(f"CFG expects label batch size {n}, but got {class_labels.shape[0]}.")
    buf = torch.empty(((2 * n if stacked is not None else n), *shape[1:]), dtype=torch.float32, device=latents.device)
    lo, hi = buf[:n], (buf[n:] if stacked is not None else None)
    x = latents.to(torch.float64) * tab.scale0
    x_hat, d_cur = torch.empty_like(x), torch.empty_like(x)
    evaluate = lambda e: _evaluate(net.model, cfg, guided, stacked, buf, n, tab.steps, e, net.img_channels, kwargs)
    for i in range(tab.num_steps):
        noise = randn_like(x)                                   # drawn every step, as the composition does: the stream does not move
        ops.edm_input(x, noise if tab.noise_on[i] else None, tab.coef, i, x_hat, lo, hi)
        cond, uncond = evaluate(2 * i)
        if tab.solver == "euler" or i == tab.num_steps - 1:
            ops.edm_step(ops.STEP_EULER, net.pred_type, cond, uncond, scale, x_hat, None, tab.coef, i, x_out=x)
            continue
        ops.edm_step(ops.STEP_PREDICT, net.pred_type, cond, uncond, scale, x_hat, d_cur, tab.coef, i, model_in=lo, model_in_dup=hi)
        cond, uncond = evaluate(2 * i + 1)
        ops.edm_step(ops.STEP_CORRECT, net.pred_type, cond, uncond, scale, x_hat, d_cur, tab.coef, i, x_out=x)
    return x


@torch.no_grad()
def edm_sample(net, latents, class_labels=None, randn_like=torch.randn_like, num_steps=18, sigma_min=None, sigma_max=None, rho=7,
               solver="heun", discretization="edm", schedule="linear", scaling="none", epsilon_s=1e-3, alpha=1, S_churn=0,
               S_min=0, S_max=float("inf"), S_noise=1, fused=None, **model_kwargs):
    """x_0 from `latents` ~ N(0, I): `num_steps` Euler / Heun (2nd-order, `alpha` = 1) steps of the EDM sampler, with the
    optional "churn" noise injection (S_churn, S_min, S_max, S_noise).  Every noise level handed to the network is first
    snapped to its chain (net.round_sigma).  fused: None = the fused kernels on the GPU, False = the tensor composition
    below, True = fused or an error; same values, dtype and noise draws either way."""
    if solver not in ("euler", "heun"):
        raise ValueError(f"solver {solver!r}")
    lo, hi = _edm_sigma_range(net, discretization, sigma_min, sigma_max, epsilon_s)
    if _want_fused(fused, latents, "edm_sample", None if net.pred_type in ops.EDM_PRED else f"pred_type {net.pred_type!r}"):
        tab = _edm_tables(net, latents.device, latents.shape[0], num_steps, lo, hi, rho, solver, discretization, schedule, scaling,
                          epsilon_s, alpha, S_churn, S_min, S_max, S_noise)
        return _edm_sample_fused(net, latents, class_labels, randn_like, tab, model_kwargs)
    path, t_grid = _edm_time_grid(net, latents.device, num_steps, lo, hi, rho, discretization, schedule, scaling, epsilon_s)
    x = latents.to(torch.float64) * (path.sigma(t_grid[0]) * path.s(t_grid[0]))
    for i in range(num_steps):
        t_cur, t_next = t_grid[i], t_grid[i + 1]
        sg_cur = path.sigma(t_cur)
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= sg_cur <= S_max else 0
        t_hat = path.sigma_inv(net.round_sigma(sg_cur + gamma * sg_cur))
        x_hat = (path.s(t_hat) / path.s(t_cur) * x
                 + (path.sigma(t_hat) ** 2 - sg_cur ** 2).clip(min=0).sqrt() * path.s(t_hat) * S_noise * randn_like(x))
        h = t_next - t_hat
        d_cur = path.slope(x_hat, t_hat, net(x_hat / path.s(t_hat), path.sigma(t_hat), class_labels, **model_kwargs).to(torch.float64))
        if solver == "euler" or i == num_steps - 1:
            x = x_hat + h * d_cur
            continue
        t_mid = t_hat + alpha * h
        x_mid = x_hat + alpha * h * d_cur
        d_mid = path.slope(x_mid, t_mid, net(x_mid / path.s(t_mid), path.sigma(t_mid), class_labels, **model_kwargs).to(torch.float64))
        x = x_hat + h * ((1 - 1 / (2 * alpha)) * d_cur + 1 / (2 * alpha) * d_mid)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# linear multistep solvers in the data-prediction form: one network evaluation per step
# ---------------------------------------------------------------------------------------------------------------------
DPM_SOLVERS = ("dpmpp2m", "dpmpp2m_sde", "expab")


def _expab_weights(lam, lam_next):
    """The weights b_j of the exponential Adams-Bashforth step from lam[0] to lam_next (lam: the nodes, newest first, 0-dim
    tensors or numbers):  sum_j b_j p(lam[j]) = int_{lam[0]}^{lam_next} e^{-(lam_next - tau)} p(tau) dtau  for every polynomial p
    of degree < len(lam) <= 3.  With u = tau - lam[0] the moments of the kernel are I_0 = -expm1(-h), I_k = h^k - k I_{k-1};
    the weights integrate the Lagrange basis over the nodes u_0 = 0, u_j = lam[j] - lam[0]."""
    lam = [torch.as_tensor(v, dtype=torch.float64) for v in lam]
    h = torch.as_tensor(lam_next, dtype=torch.float64) - lam[0]
    I0 = -torch.expm1(-h)
    if len(lam) == 1:
        return [I0]
    I1 = h - I0
    u1 = lam[1] - lam[0]
    if len(lam) == 2:
        b1 = I1 / u1
        return [I0 - b1, b1]
    I2 = h ** 2 - 2 * I1
    u2 = lam[2] - lam[0]
    return [(I2 - (u1 + u2) * I1 + u1 * u2 * I0) / (u1 * u2), (I2 - u2 * I1) / (u1 * (u1 - u2)), (I2 - u1 * I1) / (u2 * (u2 - u1))]


def _dpm_2m_weights(sig_cur, sig_next, h, h_last, eta, s_noise):
    """(a, b0, b1, c) of the DPM-Solver++(2M) step in its midpoint form, h_last=None: the first-order step.  One routine for
    the deterministic solver (eta = 0: a = sig_next / sig_cur, J = -expm1(-h), c = 0) and its SDE variant."""
    eta_h = eta * h
    a = sig_next / sig_cur * torch.exp(-eta_h)
    J = -torch.expm1(-h - eta_h)
    c = sig_next * torch.sqrt(-torch.expm1(-2 * eta_h)) * s_noise
    if h_last is None:
        return a, J, 0.0, c
    w = 1 / (2 * (h_last / h))
    return a, J * (1 + w), -(J * w), c


def _dpm_tables(net, device, batch, num_steps, lo, hi, rho, solver, order, discretization, epsilon_s, eta, s_noise):
    """Everything of dpm_sample's loop that does not depend on x, computed once per grid in float64 on `device` and cached on
    the denoiser:
      sigma   [num_steps + 1] float64: the snapped noise levels, then 0
      coef    [num_steps, ops.DPM_COLS] float64 on the device (include/vaw_hip.h): a, b0, b1, b2, c of
              x' = a x + b0 D0 + b1 D1 + b2 D2 + c noise, then the float32 scalars of EDMDenoiser.forward at this evaluation
              (sigma, c_in, c_in^2, sigma c_in) widened, then c_in of the next evaluation
      steps   [num_steps, 2 * batch] int32 on the device: the chain index handed to the network (a guided call takes a whole
              row, any other its first half)
      nodes, noise_on, t_mean   host lists: how many denoised images step i combines (1..3), whether it adds noise, and the
              mean timestep as the network sees it (the argument of the guidance predicate), from one read-back.
    For a denoiser that only follows the protocol (no chain: an analytic D(x; sigma)) the evaluation columns stay zero and
    steps / t_mean are None: the composition needs neither.  Raises ValueError where two adjacent snapped levels do not decrease."""
    key = ("dpm", solver, order, num_steps, discretization, float(lo), float(hi), rho, epsilon_s, float(eta), float(s_noise), int(batch),
           str(device))
    cache = net.__dict__.setdefault("_solver_tables", {})
    if key in cache:
        return cache[key]
    sig = net.round_sigma(_noise_levels(net, discretization, num_steps, lo, hi, rho, epsilon_s, device))
    sig = torch.cat([sig, torch.zeros_like(sig[:1])])
    lam = -sig[:num_steps].log()
    chain = hasattr(net, "nearest_index") and hasattr(net, "M")

    def evaluation(sigma64):
        sigma = sigma64.to(torch.float32).reshape(-1, 1, 1, 1)               # EDMDenoiser.forward
        c_in = 1 / (sigma ** 2 + 1).sqrt()
        step = (net.M - 1 - net.nearest_index(sigma).to(torch.float32)).flatten()
        return [sigma, c_in, c_in ** 2, sigma * c_in], step

    rows, steps, t_mean, nodes = [], [], [], []
    for i in range(num_steps):
        last = i == num_steps - 1
        q = 1 if last or i == 0 else 2 if solver != "expab" else min(order, i + 1)
        if last:                                                              # sigma_next = 0: x' = D0
            w = [0.0, 1.0, 0.0, 0.0, 0.0]
        elif solver == "expab":
            b = _expab_weights([lam[i - j] for j in range(q)], lam[i + 1])
            w = [sig[i + 1] / sig[i], *b, *([0.0] * (3 - q)), 0.0]
        else:
            h = lam[i + 1] - lam[i]
            a, b0, b1, c = _dpm_2m_weights(sig[i], sig[i + 1], h, lam[i] - lam[i - 1] if q == 2 else None, eta, s_noise)
            w = [a, b0, b1, 0.0, c]
        ev = [0.0] * 5
        if chain:
            scalars, step = evaluation(sig[i])
            ev = scalars + [0.0 if last else evaluation(sig[i + 1])[0][1]]
            steps.append(step.repeat(2 * batch).int())
            t_mean.append(steps[-1][:batch].float().mean())                  # IntervalCFG.forward's read-back
        rows.append(_row(w + ev, torch.float64, device, ops.DPM_COLS))
        nodes.append(q)
    coef = torch.stack(rows).contiguous()
    host = torch.cat([sig, torch.stack(t_mean).to(torch.float64)] if chain else [sig]).tolist()
    for i in range(num_steps):
        if not host[i] > host[i + 1]:
            raise ValueError(f"dpm_sample: the snapped noise levels do not decrease at step {i} (sigma {host[i]!r} -> {host[i + 1]!r}): "
                             "h <= 0 there; use fewer steps or another discretization")
    tab = SimpleNamespace(coef=coef, sigma=sig, steps=torch.stack(steps).contiguous() if chain else None, nodes=nodes,
                          noise_on=[solver == "dpmpp2m_sde" and eta > 0 and i < num_steps - 1 for i in range(num_steps)],
                          t_mean=host[num_steps + 1:] if chain else [None] * num_steps, solver=solver, num_steps=num_steps)
    cache[key] = tab
    return tab


def _dpm_sample_fused(net, latents, class_labels, randn_like, tab, clip_denoised, model_kwargs):
    """dpm_sample's loop on the fused kernels: vaw_dpm_input once, then per step the network, the noise draw where the step
    adds noise, and vaw_dpm_step, which also writes the next network input.  The float32 denoised images of the last three
    steps live in three buffers rotated by reference.  No host synchronisation."""
    n, shape = latents.shape[0], tuple(latents.shape)
    kwargs = {**model_kwargs, "y": class_labels}
    cfg, guided, scale, stacked = _guidance(net.model, class_labels, tab.t_mean, kwargs)
    if stacked is not None and class_labels.shape[0] != n:
        raise AssertionError(f"CFG expects label batch size {n}, but got {class_labels.shape[0]}.")
    buf = torch.empty(((2 * n if stacked is not None else n), *shape[1:]), dtype=torch.float32, device=latents.device)
    lo, hi = buf[:n], (buf[n:] if stacked is not None else None)
    x = latents.to(torch.float64) * tab.sigma[0]
    hist = [torch.empty(shape, dtype=torch.float32, device=latents.device) for _ in range(3)]          # D0 (written), D1, D2
    ops.dpm_input(x, tab.coef, 0, lo, hi)
    for i in range(tab.num_steps):
        cond, uncond = _evaluate(net.model, cfg, guided, stacked, buf, n, tab.steps, i, net.img_channels, kwargs)
        noise = randn_like(x) if tab.noise_on[i] else None
        more = i < tab.num_steps - 1
        ops.dpm_step(net.pred_type, clip_denoised, cond, uncond, scale, x, hist[1] if tab.nodes[i] >= 2 else None,
                     hist[2] if tab.nodes[i] >= 3 else None, noise, tab.coef, i, x_out=x, d0_out=hist[0],
                     model_in=lo if more else None, model_in_dup=hi if more else None)
        hist = [hist[2], hist[0], hist[1]]
    return x


@torch.no_grad()
def dpm_sample(net, latents, class_labels=None, randn_like=torch.randn_like, num_steps=18, sigma_min=None, sigma_max=None, rho=7,
               solver="dpmpp2m", order=None, discretization="edm", eta=1.0, s_noise=1.0, clip_denoised=False, epsilon_s=1e-3,
               fused=None, **model_kwargs):
    """x_0 (float64) from `latents` ~ N(0, I) with a linear multistep solver in the data-prediction form: ONE evaluation of
    `net` (an EDMDenoiser, or anything with net(x, sigma, labels, **kw), round_sigma, sigma_min, sigma_max) per step, on the
    noise levels of edm_sample (schedule "linear", scaling "none": sigma(t) = t, s = 1), the last step landing on sigma = 0.
    With lambda = -log sigma, h = lambda_{i+1} - lambda_i, r = h_last / h:
      solver="dpmpp2m"      DPM-Solver++(2M), midpoint form: x' = (sigma_{i+1} / sigma_i) x - expm1(-h) ((1 + 1/(2r)) D0 - 1/(2r) D1),
                            first step first order
      solver="dpmpp2m_sde"  its stochastic variant, eta_h = eta h, J = -expm1(-h - eta_h):
                            x' = (sigma_{i+1} / sigma_i) e^{-eta_h} x + J (1 + 1/(2r)) D0 - J/(2r) D1
                                 + sigma_{i+1} sqrt(-expm1(-2 eta_h)) s_noise noise;   eta = 0 is dpmpp2m, coefficient for coefficient
      solver="expab"        exponential Adams-Bashforth of `order` 1..3 (default 3): x' = (sigma_{i+1} / sigma_i) x + the exact
                            integral of e^{-(lambda_{i+1} - tau)} P(tau), P the Lagrange polynomial through the last
                            min(order, i + 1) denoised images (`_expab_weights`)
    and x' = D0 on the last step.  The coefficients a, b0, b1, b2, c of a step are computed once per grid (`_dpm_tables`);
    the update is acc = a x + b0 D0, then + b1 D1, + b2 D2, + c noise where the step has them, every operation rounded on
    its own in float64, D the float32 denoised image (clamped to [-1, 1] with clip_denoised) widened.  randn_like(x) is drawn
    once per step that adds noise (dpmpp2m_sde with eta > 0, all steps but the last).  fused: as in edm_sample (None =
    vaw_dpm_input / vaw_dpm_step on the GPU, bitwise the composition below)."""
    if solver not in DPM_SOLVERS:
        raise ValueError(f"solver {solver!r} (one of {DPM_SOLVERS})")
    if solver == "expab":
        order = 3 if order is None else order
        if order not in (1, 2, 3):
            raise ValueError(f"dpm_sample: order {order!r} of expab is not 1, 2 or 3")
    elif order is not None:
        raise ValueError(f"dpm_sample: order is a parameter of solver 'expab', not of {solver!r} (second order)")
    if eta < 0 or s_noise < 0:
        raise ValueError(f"dpm_sample: eta {eta!r} and s_noise {s_noise!r} must not be negative")
    if num_steps < 2:
        raise ValueError(f"dpm_sample: num_steps {num_steps!r} < 2")
    if solver != "dpmpp2m_sde":
        eta, s_noise = 0.0, 1.0
    lo, hi = _edm_sigma_range(net, discretization, sigma_min, sigma_max, epsilon_s)
    pred_type = getattr(net, "pred_type", None)
    unsupported = (None if pred_type in ops.EDM_PRED and hasattr(net, "nearest_index") else
                   f"pred_type {pred_type!r}" if pred_type is not None else "a denoiser without EDMDenoiser's chain")
    use = _want_fused(fused, latents, "dpm_sample", unsupported)
    tab = _dpm_tables(net, latents.device, latents.shape[0], num_steps, lo, hi, rho, solver, order, discretization, epsilon_s, eta, s_noise)
    if use:
        return _dpm_sample_fused(net, latents, class_labels, randn_like, tab, clip_denoised, model_kwargs)
    x = latents.to(torch.float64) * tab.sigma[0]
    hist = []
    for i in range(num_steps):
        d0 = net(x, tab.sigma[i], class_labels, **model_kwargs)
        if clip_denoised:
            d0 = d0.clamp(-1, 1)
        a, b0, b1, b2, c = tab.coef[i, :5].unbind()
        acc = a * x + b0 * d0.to(torch.float64)
        if tab.nodes[i] >= 2:
            acc = acc + b1 * hist[0].to(torch.float64)
        if tab.nodes[i] >= 3:
            acc = acc + b2 * hist[1].to(torch.float64)
        if tab.noise_on[i]:
            acc = acc + c * randn_like(x)
        x = acc
        hist = [d0] + hist[:1]
    return x


# ---------------------------------------------------------------------------------------------------------------------
# flow matching
# ---------------------------------------------------------------------------------------------------------------------
def _flow_fields(fm, out, x_t, t):
    """(velocity field, score) implied by the model output at (x_t, t) under fm's parametrisation and interpolant
    (reference convert_model_output_to_vector / _to_score, gaussian_diffusion.py:1205-1257)."""
    a, s, da, ds = fm.interpolant(t)
    mt = fm.model_mean_type
    if mt == ModelMeanType.START_X:
        x0 = out
        eps = (x_t - a * x0) / s
        score = -(x_t - a * x0) / (s ** 2)
    elif mt == ModelMeanType.EPSILON:
        eps = out
        x0 = (x_t - s * eps) / a
        score = -eps / s
    elif mt == ModelMeanType.VELOCITY:
        den = a ** 2 + s ** 2
        x0 = (a * x_t - s * out) / den
        eps = (s * x_t + a * out) / den
        score = -eps / s
    elif mt == ModelMeanType.VECTOR:
        eps = (da * x_t - a * out) / (s * da - a * ds)
        return out, -eps / s
    elif mt == ModelMeanType.SCORE:
        raise NotImplementedError("Unsupported model_mean_type for vector")        # as the reference: a score model has no vector map
    else:
        raise NotImplementedError(f"Unsupported model_mean_type {mt}")
    return da * x0 + ds * eps, score


def _flow_eval(fm, model, x, t_scalar, model_kwargs):
    t = fm.expand_t_like_x(t_scalar, x)
    out = _unwrap(model(x, t.view(x.shape[0]), **model_kwargs))
    return t, out


def _flow_tables(fm, kind, solver, num_steps, batch, device):
    """What the flow loops compute per evaluation that does not depend on x, with their own expressions, cached on `fm`:
      coef   [evaluations, ops.FLOW_COLS] float32 on the device (include/vaw_hip.h): the interpolant at t and what
             _flow_fields / the drift derive from it, and dt, sqrt|dt|, dt/2 of the step that starts there
      times  [evaluations, 2 * batch] float32 on the device: t as the network gets it (a guided call takes a whole row)
      t_mean host list: the mean of the first half of each row, the argument of the guidance predicate.
    kind "sde": per step the evaluation at t_k (and t_{k+1} for Heun), then the last noise-free step; "ode": the same
    without the last one."""
    key = (kind, solver, num_steps, fm.path_type, int(batch), str(device))
    cache = fm.__dict__.setdefault("_solver_tables", {})
    if key in cache:
        return cache[key]
    if kind == "sde":
        grid = torch.cat([torch.linspace(1.0, 0.04, num_steps, dtype=torch.float64, device=device),
                          torch.zeros(1, dtype=torch.float64, device=device)])
    else:
        grid = torch.linspace(1.0, 0.0, num_steps, device=device)
    like = torch.empty((batch, 1, 1, 1), dtype=torch.float32, device=device)
    rows, times, t_mean = [], [], []

    def evaluation(t_scalar, dt):
        tb = fm.expand_t_like_x(t_scalar, like)                    # _flow_eval
        t = tb[:1]
        a, s, da, ds = fm.interpolant(t)
        g2 = 2 * s * ds
        step = [0.0, 0.0, 0.0] if dt is None else [dt, torch.sqrt(torch.abs(dt)), 0.5 * dt]
        rows.append(_row([a, s, da, ds, g2, 0.5 * g2, s ** 2, a ** 2 + s ** 2, s * da - a * ds, torch.sqrt(g2), *step, t],
                         torch.float32, device, ops.FLOW_COLS))
        times.append(tb.view(batch).repeat(2))
        t_mean.append(tb.view(batch).float().mean())              # IntervalCFG.forward's read-back

    for k in range(num_steps - 1):
        evaluation(grid[k], grid[k + 1] - grid[k])
        if solver == "heun":
            evaluation(grid[k + 1], None)
    if kind == "sde":
        evaluation(grid[-2], grid[-1] - grid[-2])
    tab = SimpleNamespace(coef=torch.stack(rows).contiguous(), times=torch.stack(times).contiguous(),
                          t_mean=torch.stack(t_mean).tolist(), solver=solver, num_steps=num_steps)
    cache[key] = tab
    return tab


def _flow_sample_fused(fm, model, noise, randn_like, tab, sde, model_kwargs):
    """The Euler / Heun loops of flow_sde_sample and flow_ode_sample on vaw_flow_step.  x lives in the first half of one of
    three network-input buffers (current, Heun prediction, next), so every step writes the next network input directly."""
    n, shape = noise.shape[0], tuple(noise.shape)
    y = model_kwargs.get("y")
    cfg, guided, scale, stacked = _guidance(model, y, tab.t_mean, model_kwargs)
    if stacked is not None and y.shape[0] != n:
        raise AssertionError(f"CFG expects label batch size {n}, but got {y.shape[0]}.")
    rows = 2 * n if stacked is not None else n
    cur, pred, nxt = (torch.empty((rows, *shape[1:]), dtype=torch.float32, device=noise.device) for _ in range(3))
    half = lambda b: (b[:n], b[n:] if stacked is not None else None)
    for part in half(cur):
        if part is not None:
            part.copy_(noise)
    f0 = torch.empty(shape, dtype=torch.float32, device=noise.device)
    kick = torch.empty_like(f0) if sde else None
    mean_type = fm.model_mean_type.name
    evaluate = lambda e, buf: _evaluate(model, cfg, guided, stacked, buf, n, tab.times, e, None, model_kwargs)
    e = 0
    for _ in range(tab.num_steps - 1):
        cond, uncond = evaluate(e, cur)
        z = randn_like(cur[:n]) if sde else None
        if tab.solver == "euler":
            ops.flow_step(ops.STEP_EULER, sde, mean_type, cond, uncond, scale, cur[:n], z, None, None, None, tab.coef, e, e, *half(nxt))
            e += 1
        else:
            ops.flow_step(ops.STEP_PREDICT, sde, mean_type, cond, uncond, scale, cur[:n], z, None, f0, kick, tab.coef, e, e + 1, *half(pred))
            cond, uncond = evaluate(e + 1, pred)
            ops.flow_step(ops.STEP_CORRECT, sde, mean_type, cond, uncond, scale, cur[:n], None, pred[:n], f0, kick, tab.coef, e, e + 1,
                          *half(nxt))
            e += 2
        cur, nxt = nxt, cur
    if sde:
        cond, uncond = evaluate(e, cur)
        ops.flow_step(ops.STEP_EULER, sde, mean_type, cond, uncond, scale, cur[:n], None, None, None, None, tab.coef, e, e, nxt[:n])
        cur = nxt
    return cur[:n]


def _flow_unsupported(fm, noise, solver):
    if fm.model_mean_type.name not in ops.FLOW_MEAN:
        return f"model_mean_type {fm.model_mean_type}"
    if solver not in ("euler", "heun"):
        return f"solver {solver!r} (euler and heun are fused)"
    if noise.dtype != torch.float32:
        return f"{noise.dtype} noise"
    return None


# ---- adaptive Dormand-Prince 5(4) ---------------------------------------------------------------------------------------------
# The tableau (C, A with B = A[6], error weights E) and the controller's constants, as scipy.integrate's RK45 has them.
_DP_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_A = ((),
         (1 / 5,),
         (3 / 40, 9 / 40),
         (44 / 45, -56 / 15, 32 / 9),
         (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
         (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)
_RK_SAFETY, _RK_MIN_FACTOR, _RK_MAX_FACTOR, _RK_EXPONENT = 0.9, 0.2, 10.0, -1 / 5


def _ode_tolerances(fm, rtol, atol):
    """rtol / atol of the adaptive solver: the keyword, then fm's attribute, then fm.args', then the reference's defaults."""
    def pick(name, given, default):
        for v in (given, getattr(fm, name, None), getattr(getattr(fm, "args", None), name, None)):
            if v is not None:
                return float(v)
        return default
    return pick("rtol", rtol, 1e-3), pick("atol", atol, 1e-6)


def _rk_combine(coeffs, k):
    """sum_j coeffs[j] * k[j] in float32: ascending, zero coefficients skipped, left to right (None if all are zero)."""
    dy = None
    for c, kj in zip(coeffs, k):
        if c != 0:
            dy = c * kj if dy is None else dy + c * kj
    return dy


def _rk_sumsq(u, scale):
    """sum (u / scale)^2: the quotient in u's dtype (float32), squares and sum in float64, as a Python float."""
    return float(((u / scale).to(torch.float64) ** 2).sum())


class _RK45Composition:
    """The arithmetic of an adaptive step as tensor operations (any device): what the fused kernels are checked against."""

    def __init__(self, fm, model, noise, rtol, atol, model_kwargs):
        self.fm, self.model, self.kwargs, self.rtol, self.atol = fm, model, model_kwargs, rtol, atol
        self.x, self.k, self.nfev, self.readbacks = noise, [None] * 7, 0, 0

    def drift(self, x, t):
        self.nfev += 1
        tb, out = _flow_eval(self.fm, self.model, x, torch.tensor(t, dtype=torch.float64, device=x.device), self.kwargs)
        return _flow_fields(self.fm, out, x, tb)[0]

    def start(self, t):
        self.k[0] = self.drift(self.x, t)
        scale = self.atol + self.rtol * self.x.abs()
        self.readbacks += 1
        return _rk_sumsq(self.x, scale), _rk_sumsq(self.k[0], scale)

    def trial(self, t, h):
        f1 = self.drift(self.x + h * _rk_combine((1.0,), self.k), t + h)
        self.readbacks += 1
        return _rk_sumsq(f1 - self.k[0], self.atol + self.rtol * self.x.abs())

    def attempt(self, t, h, t_new, have_k1):
        x, k = self.x, self.k
        if not have_k1:
            k[0] = self.drift(x, t)
        for i in range(1, 7):
            xi = x + h * _rk_combine(_DP_A[i], k)
            k[i] = self.drift(xi, t + _DP_C[i] * h if i < 6 else t_new)
        self.x_new = xi
        err = h * _rk_combine(_DP_E, k)
        self.readbacks += 1
        return _rk_sumsq(err, self.atol + self.rtol * torch.maximum(x.abs(), xi.abs()))

    def accept(self):
        self.x, self.k[0] = self.x_new, self.k[6]

    def result(self):
        return self.x


class _RK45Fused:
    """The same on vaw_rk_stage / vaw_rk_scaled_sumsq.  x lives in the first half of a network-input buffer (`cur`), the
    stage states go straight into another (`stg`), the seventh into a third (`new`), which is the next x: accepting a step
    swaps `cur` and `new` and the slots of k1 and k7, and copies nothing.  Per attempt: one upload of the seven stage times,
    the interpolant table computed from them on the device with the expressions of _flow_tables, the (network, vaw_rk_stage)
    pairs, and one 8-byte read-back of the error's sum of squares."""

    def __init__(self, fm, model, noise, rtol, atol, model_kwargs):
        n, shape, dev = noise.shape[0], tuple(noise.shape), noise.device
        self.fm, self.model, self.kwargs, self.rtol, self.atol, self.n = fm, model, model_kwargs, rtol, atol, n
        y = model_kwargs.get("y")
        cfg = model if hasattr(model, "guided_halves") else None
        self.cfg, self.scale = cfg, (cfg.guidance_scale if cfg is not None else 1.0)
        self.can = cfg is not None and cfg.class_cond and y is not None
        self.stacked = None
        if self.can and cfg.guidance_active(sum(cfg.interval) / 2):          # the scale alone can switch guidance off for good
            if y.shape[0] != n:
                raise AssertionError(f"CFG expects label batch size {n}, but got {y.shape[0]}.")
            self.stacked = {**model_kwargs, "y": torch.cat((y, y.new_full(y.shape, cfg.null_label)))}
        rows = 2 * n if self.stacked is not None else n
        self.cur, self.stg, self.new = (torch.empty((rows, *shape[1:]), dtype=torch.float32, device=dev) for _ in range(3))
        for part in self.half(self.cur):
            if part is not None:
                part.copy_(noise)
        self.k = torch.empty((ops.RK_STAGES, *shape), dtype=torch.float32, device=dev)
        self.slots = list(range(ops.RK_STAGES))
        self.count = ops.rk_partial_count(n, noise[0].numel())
        self.partials = torch.empty(self.count, dtype=torch.float64, device=dev)
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.mean_type = fm.model_mean_type.name
        self.nfev, self.readbacks = 0, 0

    def half(self, buf):
        return buf[:self.n], (buf[self.n:] if self.stacked is not None else None)

    def tables(self, times):
        """For the stage times (host float64): the [len, FLOW_COLS] table on the device, the [len, 2n] float32 times the
        network gets, and the guidance predicate of each on the host, from the float32 time."""
        dev = self.cur.device
        t = torch.tensor(times, dtype=torch.float64).to(dev).to(torch.float32).view(-1, 1)          # the one upload; expand_t_like_x
        a, s, da, ds = self.fm.interpolant(t)
        g2 = 2 * s * ds
        zero = torch.zeros_like(t)
        cols = [a, s, da, ds, g2, 0.5 * g2, s ** 2, a ** 2 + s ** 2, s * da - a * ds, torch.sqrt(g2), zero, zero, zero, t, zero, zero]
        guided = [self.stacked is not None and self.cfg.guidance_active(float(np.float32(tm))) for tm in times]
        return torch.cat(cols, 1).contiguous(), t.repeat(1, 2 * self.n), guided

    def evaluate(self, tab, e, buf):
        self.nfev += 1
        coef, times, guided = tab
        return _evaluate(self.model, self.cfg, guided, self.stacked, buf, self.n, times, e, None, self.kwargs)

    def stage(self, i, out, tab, row, x_stage, coeffs, h, x_out=None, partials=False):
        cond, uncond = out if out is not None else (None, None)
        lo, hi = self.half(x_out) if x_out is not None else (None, None)
        ops.rk_stage(i, self.mean_type, cond, uncond, self.scale, self.cur[:self.n], x_stage, tab[0] if tab is not None else None, row,
                     self.k, self.slots, coeffs, h, lo, hi, self.new[:self.n] if partials else None, self.atol, self.rtol,
                     self.partials if partials else None)

    def sumsq(self, u, v, slot):
        ops.rk_scaled_sumsq(u, v, self.cur[:self.n], None, self.atol, self.rtol, self.partials)
        ops.rk_sumsq_finish(self.partials, self.count, self.sums[slot:])

    def start(self, t):
        tab = self.tables([t])
        self.stage(0, self.evaluate(tab, 0, self.cur), tab, 0, None, (), 0.0)
        self.sumsq(self.cur[:self.n], None, 0)
        self.sumsq(self.k[self.slots[0]], None, 1)
        self.readbacks += 1
        return tuple(self.sums.tolist())

    def trial(self, t, h):
        tab = self.tables([t + h])
        self.stage(0, None, None, 0, None, (1.0,), h, x_out=self.stg)
        self.stage(1, self.evaluate(tab, 0, self.stg), tab, 0, self.stg[:self.n], (), 0.0)
        self.sumsq(self.k[self.slots[1]], self.k[self.slots[0]], 0)
        self.readbacks += 1
        return self.sums[0].item()

    def attempt(self, t, h, t_new, have_k1):
        tab = self.tables([t + c * h for c in _DP_C[:6]] + [t_new])
        self.stage(0, None if have_k1 else self.evaluate(tab, 0, self.cur), tab, 0, None, _DP_A[1], h, x_out=self.stg)
        for i in range(1, 6):
            self.stage(i, self.evaluate(tab, i, self.stg), tab, i, self.stg[:self.n], _DP_A[i + 1], h,
                       x_out=self.stg if i < 5 else self.new)
        self.stage(6, self.evaluate(tab, 6, self.new), tab, 6, self.new[:self.n], _DP_E, h, partials=True)
        ops.rk_sumsq_finish(self.partials, self.count, self.sums)
        self.readbacks += 1
        return self.sums[0].item()

    def accept(self):
        self.cur, self.new = self.new, self.cur
        self.slots[0], self.slots[6] = self.slots[6], self.slots[0]

    def result(self):
        return self.cur[:self.n].clone()


def _rk45_integrate(fm, be, n_elems, max_attempts):
    """From t = 1 to t = 0 with the step controller of scipy's RK45, in Python float64 on the host; `be` does the tensor work
    and hands back sums of squares.  The batch is one system with one step size.  Every attempt is clipped to land on the
    end exactly: the network is never evaluated beyond it and nothing is interpolated.  The first attempt evaluates its first
    stage itself (the launch that writes the second stage's state needs h, which the first-step selection finds from that
    same evaluation), every later one gets it from the step before: 2 + 6 * attempts + 1 network evaluations."""
    t, t_end, direction = 1.0, 0.0, -1.0
    interval = abs(t_end - t)
    rms = lambda sumsq: math.sqrt(sumsq / n_elems)
    # first step (Hairer, Norsett, Wanner I, II.4; scipy's select_initial_step with the order of the error estimator, 4)
    d0, d1 = (rms(v) for v in be.start(t))
    if not (math.isfinite(d0) and math.isfinite(d1)):
        raise FloatingPointError(f"flow_ode_sample: non-finite state or drift at t={t} (before the first step, h undefined)")
    h0 = min(1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1, interval)
    d2 = rms(be.trial(t, direction * h0)) / h0
    if not math.isfinite(d2):
        raise FloatingPointError(f"flow_ode_sample: non-finite drift in the first-step trial at t={t}, h={direction * h0}")
    h1 = max(1e-6, h0 * 1e-3) if d1 <= 1e-15 and d2 <= 1e-15 else (0.01 / max(d1, d2)) ** (1 / 5)
    h_abs = min(100 * h0, h1, interval)
    stats = dict(accepted=0, rejected=0, nfev=0, readbacks=0, h_min=math.inf, h_max=0.0, trace=[])
    fm.last_ode_stats = stats
    attempts, have_k1 = 0, False
    try:
        while direction * (t - t_end) < 0:
            min_step = 10 * abs(float(np.nextafter(t, direction * np.inf)) - t)
            h_abs = max(h_abs, min_step)
            step_rejected = False
            while True:
                if h_abs < min_step:
                    raise RuntimeError(f"flow_ode_sample: the step size fell below the spacing of t at t={t} (h={h_abs})")
                if attempts >= max_attempts:
                    raise RuntimeError(f"flow_ode_sample: more than max_attempts={max_attempts} attempts (t={t}, h={h_abs})")
                t_new = t + h_abs * direction
                if direction * (t_new - t_end) > 0:
                    t_new = t_end
                h = t_new - t
                h_abs = abs(h)
                attempts += 1
                sumsq = be.attempt(t, h, t_new, have_k1)
                have_k1 = True
                norm = rms(sumsq) if math.isfinite(sumsq) else math.nan
                stats["trace"].append((t, h, norm))
                if not math.isfinite(norm):
                    raise FloatingPointError(f"flow_ode_sample: non-finite error norm at t={t}, h={h}")
                if norm < 1:
                    factor = _RK_MAX_FACTOR if norm == 0 else min(_RK_MAX_FACTOR, _RK_SAFETY * norm ** _RK_EXPONENT)
                    if step_rejected:
                        factor = min(1.0, factor)
                    stats["accepted"] += 1
                    stats["h_min"], stats["h_max"] = min(stats["h_min"], h_abs), max(stats["h_max"], h_abs)
                    h_abs *= factor
                    be.accept()
                    t = t_new
                    break
                h_abs *= max(_RK_MIN_FACTOR, _RK_SAFETY * norm ** _RK_EXPONENT)
                step_rejected = True
                stats["rejected"] += 1
    finally:
        stats["nfev"], stats["readbacks"] = be.nfev, be.readbacks
    return be.result()


@torch.no_grad()
def flow_sde_sample(fm, model, noise, device=None, num_steps=50, solver="heun", randn_like=torch.randn_like, fused=None, **model_kwargs):
    """Reverse-time SDE of the flow (reference sde_sample :1374-1409): drift = v - (1/2) g^2 score with g^2 = 2 sigma_t sigma_t',
    Euler-Maruyama or its Heun (trapezoidal drift) variant on t = linspace(1, 0.04, num_steps) in float64, and one final
    noise-free Euler step from 0.04 to 0.  fused: as in edm_sample (None = vaw_flow_step on the GPU, bitwise this composition)."""
    if solver not in ("euler", "heun"):
        raise ValueError(f"Unknown solver: {solver}")
    if _want_fused(fused, noise, "flow_sde_sample", _flow_unsupported(fm, noise, solver)):
        return _flow_sample_fused(fm, model, noise, randn_like, _flow_tables(fm, "sde", solver, num_steps, noise.shape[0], noise.device),
                                  True, model_kwargs)
    dev = noise.device
    grid = torch.cat([torch.linspace(1.0, 0.04, num_steps, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)])

    def drift_at(x, t_scalar):
        t, out = _flow_eval(fm, model, x, t_scalar, model_kwargs)
        _, s, _, ds = fm.interpolant(t)
        g2 = 2 * s * ds
        v, score = _flow_fields(fm, out, x, t)
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


@torch.no_grad()
def flow_ode_sample(fm, model, noise, device=None, num_steps=50, solver="heun", fused=None, rtol=None, atol=None, max_attempts=1000,
                    **model_kwargs):
    """Probability-flow ODE dx/dt = v(x, t) from t = 1 to 0: with a FIXED-grid solver, euler | midpoint | heun | rk4, on the
    reference's grid linspace(1, 0, num_steps) (ode_sample :1355-1366), or adaptively with solver="rk45" (Dormand-Prince
    5(4) under scipy's RK45 step controller, `_rk45_integrate`), which ignores num_steps and takes rtol / atol: the keyword,
    else fm.rtol / fm.atol, else fm.args.rtol / fm.args.atol, else 1e-3 / 1e-6 (the reference's sample.py defaults) -- and
    leaves fm.last_ode_stats = {accepted, rejected, nfev, readbacks, h_min, h_max (accepted steps), trace: (t, h, error
    norm) of every attempt}.  It raises instead of looping: FloatingPointError on a non-finite error norm, RuntimeError when
    the step falls below the spacing of t or after max_attempts attempts.  The reference hands the same drift to torchdiffeq.odeint (dopri5 by
    default); `dopri5` stays refused because equality with torchdiffeq's steps cannot be pinned here.  Mean types whose
    conversion is singular at an end of the interval (EPSILON on the linear path at t = 1, START_X at t = 0) are the
    caller's business, as in the reference.  fused: as in edm_sample, for euler, heun and rk45 (midpoint and rk4 stay the
    tensor composition; fused=True refuses them)."""
    if solver == "dopri5":
        raise NotImplementedError("flow_ode_sample: the adaptive dopri5 of torchdiffeq (not installed; parity unpinned) is not "
                                  "restated; use solver='rk45' (the same Dormand-Prince pair under scipy's step controller) or "
                                  "euler | midpoint | heun | rk4 on the fixed grid")
    if solver == "rk45":
        rtol, atol = _ode_tolerances(fm, rtol, atol)
        use = _want_fused(fused, noise, "flow_ode_sample", _flow_unsupported(fm, noise, "euler"))
        backend = (_RK45Fused if use else _RK45Composition)(fm, model, noise, rtol, atol, model_kwargs)
        return _rk45_integrate(fm, backend, noise.numel(), max_attempts)
    if solver not in ("euler", "midpoint", "heun", "rk4"):
        raise ValueError(f"Unknown solver: {solver}")
    if _want_fused(fused, noise, "flow_ode_sample", _flow_unsupported(fm, noise, solver)):
        return _flow_sample_fused(fm, model, noise, None, _flow_tables(fm, "ode", solver, num_steps, noise.shape[0], noise.device),
                                  False, model_kwargs)
    grid = torch.linspace(1.0, 0.0, num_steps, device=noise.device)

    def v(x, t_scalar):
        t, out = _flow_eval(fm, model, x, t_scalar, model_kwargs)
        return _flow_fields(fm, out, x, t)[0]

    x = noise
    for k in range(num_steps - 1):
        t0, t1 = grid[k], grid[k + 1]
        dt = t1 - t0
        k1 = v(x, t0)
        if solver == "euler":
            x = x + dt * k1
        elif solver == "midpoint":
            x = x + dt * v(x + 0.5 * dt * k1, t0 + 0.5 * dt)
        elif solver == "heun":
            x = x + 0.5 * dt * (k1 + v(x + dt * k1, t1))
        else:
            k2 = v(x + 0.5 * dt * k1, t0 + 0.5 * dt)
            k3 = v(x + 0.5 * dt * k2, t0 + 0.5 * dt)
            x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + v(x + dt * k3, t1))
    return x


# ---- log-likelihood along the probability-flow ODE ----------------------------------------------------------------------------
# Explicit tableaus (c, a, b) of the fixed-grid solvers of the augmented system (state, accumulated divergence).
_LOGP_TABLEAUS = {"euler": ((0.0,), ((),), (1.0,)),
                  "heun": ((0.0, 1.0), ((), (1.0,)), (0.5, 0.5)),
                  "rk4": ((0.0, 0.5, 0.5, 1.0), ((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6))}
_LN_2PI = 1.8378770664093453


def _flow_logp_ab(fm, t):
    """(A, B) of v = A * x + B * out at time t as Python floats: the reference's convert_model_output_to_vector (`_flow_fields`)
    collapsed per mean type, from the interpolant in float64 on the host.  Not finite where the conversion is singular."""
    a, s, da, ds = (v.reshape(()) for v in fm.interpolant(torch.tensor([float(t)], dtype=torch.float64)))
    mt = fm.model_mean_type.name
    if mt == "START_X":
        A, B = ds / s, da - a * (ds / s)
    elif mt == "EPSILON":
        A, B = da / a, ds - s * (da / a)
    elif mt == "VELOCITY":
        den = a ** 2 + s ** 2
        A, B = (a * da + s * ds) / den, (a * ds - s * da) / den
    elif mt == "VECTOR":
        A, B = torch.zeros_like(a), torch.ones_like(a)
    else:
        raise ValueError(f"flow_log_likelihood: model_mean_type {mt} has no vector field in the reference")
    return float(A), float(B)


def _flow_logp_tables(fm, solver, num_steps, t_span):
    """The grid of flow_log_likelihood on the host, cached on `fm`: per network evaluation the time (float64) and (A, B)
    (float64; the float32 table the kernel reads is made from them), per step h.  Raises where A or B is not finite."""
    t_lo, t_hi = float(t_span[0]), float(t_span[1])
    key = ("logp", solver, int(num_steps), fm.path_type, fm.model_mean_type.name, t_lo, t_hi)
    cache = fm.__dict__.setdefault("_solver_tables", {})
    if key in cache:
        return cache[key]
    c, a, b = _LOGP_TABLEAUS[solver]
    grid = np.linspace(t_lo, t_hi, num_steps, dtype=np.float64)
    times, ab, hs = [], [], []
    for k in range(num_steps - 1):
        h = float(grid[k + 1] - grid[k])
        hs.append(h)
        for ci in c:
            t = float(grid[k + 1]) if ci == 1.0 else float(grid[k]) + ci * h
            A, B = _flow_logp_ab(fm, t)
            if not (math.isfinite(A) and math.isfinite(B)):
                raise ValueError(f"flow_log_likelihood: the vector field of a {fm.model_mean_type.name} model on the {fm.path_type!r} path "
                                 f"is singular at the grid time t={t} (A={A}, B={B}); move t_span off that end")
            times.append(t)
            ab.append((A, B))
    tab = SimpleNamespace(c=c, a=a, b=b, times=times, ab=ab, h=hs, solver=solver, num_steps=num_steps, device={})
    cache[key] = tab
    return tab


def _flow_logp_device(tab, rows, dtype, device):
    """(coef [evaluations, ops.FLOW_LOGP_COLS] float32, times [evaluations, rows] in `dtype`) on `device`: one upload each."""
    key = (int(rows), dtype, str(device))
    if key not in tab.device:
        coef = torch.tensor([[A, B, t, 0.0] for (A, B), t in zip(tab.ab, tab.times)], dtype=torch.float64).to(torch.float32)
        times = torch.tensor(tab.times, dtype=torch.float64).to(dtype).view(-1, 1).expand(len(tab.times), rows)
        tab.device[key] = (coef.to(device).contiguous(), times.to(device).contiguous())
    return tab.device[key]


def _logp_probes(kind, shape, dtype, device, generator):
    """The Hutchinson probes of one call: drawn once, on the generator's device (the tensor's without one)."""
    gdev = generator.device if generator is not None else device
    if kind == "rademacher":
        eps = torch.randint(0, 2, shape, generator=generator, device=gdev).to(dtype) * 2 - 1
    else:
        eps = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(dtype)
    return eps.to(device).contiguous()


def _logp_network(model, xin, t_rows, eps, model_kwargs):
    """One network evaluation and one vector-Jacobian product: (the x-shaped view of the output, g = (d out / d x)^T eps).
    `xin` is the network-input buffer itself, made a leaf; a learn_sigma model's probe is zero on its variance channels."""
    C = xin.shape[1]
    with torch.enable_grad():
        leaf = xin.detach().requires_grad_(True)
        only_dx = model.input_grad_only() if hasattr(model, "input_grad_only") else contextlib.nullcontext()
        with only_dx:
            out = _unwrap(model(leaf, t_rows, **model_kwargs))
            probe = eps.to(out.dtype)
            if out.shape[1] != C:
                probe = torch.cat((probe, probe.new_zeros((out.shape[0], out.shape[1] - C, *out.shape[2:]))), 1)
            (g,) = torch.autograd.grad(out, leaf, probe)
    return out.detach()[:, :C], g.detach()


def _logp_refusals(fm, model, solver, n_probes, probe, num_steps, model_kwargs):
    """Everything flow_log_likelihood refuses, with the reason, before anything is launched: the model to evaluate."""
    what = "flow_log_likelihood"
    if solver in ("rk45", "dopri5"):
        raise ValueError(f"{what}: solver {solver!r} is not offered: adaptive control of the augmented state (x, accumulated "
                         "divergence) is out of scope; use euler | heun | rk4 on the fixed grid")
    if solver not in _LOGP_TABLEAUS:
        raise ValueError(f"{what}: unknown solver {solver!r} (euler | heun | rk4)")
    if fm.model_mean_type.name == "SCORE":
        raise ValueError(f"{what}: model_mean_type SCORE has no vector field in the reference (convert_model_output_to_vector refuses it)")
    if int(n_probes) < 1:
        raise ValueError(f"{what}: n_probes={n_probes} (at least one Hutchinson probe)")
    if probe not in ("rademacher", "gaussian"):
        raise ValueError(f"{what}: probe {probe!r} (rademacher | gaussian)")
    if int(num_steps) < 2:
        raise ValueError(f"{what}: num_steps={num_steps} (the grid needs both ends)")
    if getattr(model, "training", False):
        raise ValueError(f"{what}: the model is in training mode (label / dropout masks would be redrawn at every evaluation and the "
                         "integrand would not be a function of (x, t)); call model.eval() first")
    if hasattr(model, "guided_halves"):
        if model.class_cond and model_kwargs.get("y") is not None and abs(model.guidance_scale - 1.0) >= 1e-8:
            raise ValueError(f"{what}: IntervalCFG with guidance_scale={model.guidance_scale}: a guided field is not the flow of a "
                             "normalised density, so its divergence integral is no log-likelihood; evaluate the wrapped model")
        model = model.model
        if getattr(model, "training", False):
            raise ValueError(f"{what}: the wrapped model is in training mode; call model.eval() first")
    if getattr(model, "compute_dtype", None) == "fp8":
        raise ValueError(f"{what}: compute_dtype='fp8' models are refused: the delayed-scaling state would move during an evaluation")
    return model


def flow_log_likelihood(fm, model, x, *, num_steps=50, solver="heun", t_span=(0.0, 1.0), n_probes=1, probe="rademacher",
                        generator=None, offset_bits=0.0, fused=None, **model_kwargs):
    """Per-sample log-likelihood of x under the flow model, by the instantaneous change of variables along the
    probability-flow ODE (the reference's convention: t = 0 data, t = 1 noise, dx/dt = v(x, t)):

        log p0(x0) = log N(x(t_hi); 0, I) + int_{t_lo}^{t_hi} div v(x(t), t) dt

    integrated together with x by `solver` = euler | heun | rk4 on linspace(t_lo, t_hi, num_steps) (float64 on the host, the
    state in x's dtype).  The divergence is estimated with Hutchinson probes: eps is drawn once per call from `generator`
    (`probe` = "rademacher": +-1, exact in bf16, or "gaussian") and held fixed over the whole integration, so the integrand is
    smooth in t; per evaluation g = (d out / d x)^T eps is one vector-Jacobian product (torch.autograd.grad; under
    model.input_grad_only() where the model has it, so no weight gradient is computed or touched) and div v = A n + B sum
    eps * g with v = A x + B out.  n_probes = K stacks K copies of the batch on the batch axis (one model call of K N rows) and
    averages their divergence rows in float64.  The reference has no counterpart; any torch module works as the model.

    Returns a dict: logp, prior_logp, delta_logp (float64 [N], nats), bpd = -logp / (n ln 2) + offset_bits (offset_bits = 7.0
    for 8-bit pixels scaled to [-1, 1]: the density of the unscaled integers), z (the state at t_hi), nfev, nvjp.

    fused: as in edm_sample.  None = vaw_flow_logp_stage / vaw_flow_logp_prior on the GPU (float32 x), False = the tensor
    composition on any device (float64 x allowed), True = fused or an error.  Refused with the reason before any launch: a
    model in training mode, an IntervalCFG whose guidance can be active, SCORE, the adaptive solvers, a grid time at which the
    field's conversion is singular (EPSILON on the linear path at t = 1, START_X at t = 0), fp8 models, n_probes < 1."""
    model = _logp_refusals(fm, model, solver, n_probes, probe, num_steps, model_kwargs)
    tab = _flow_logp_tables(fm, solver, int(num_steps), t_span)
    use = _want_fused(fused, x, "flow_log_likelihood", None if x.dtype == torch.float32 else f"{x.dtype} x")
    K, N, shape = int(n_probes), x.shape[0], tuple(x.shape)
    rows, n = K * N, x[0].numel()
    stacked = lambda v: v.repeat(K, *([1] * (v.dim() - 1))) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N and K > 1 else v
    kwargs = {name: stacked(v) for name, v in model_kwargs.items()}
    eps = _logp_probes(probe, (rows, *shape[1:]), x.dtype, x.device, generator)
    coef, times = _flow_logp_device(tab, rows, x.dtype, x.device)
    S, e = len(tab.c), 0
    stage_coeffs = lambda i: tab.b if i == S - 1 else tab.a[i + 1]
    x0 = stacked(x.detach()).contiguous()
    if use:
        bufs = [torch.empty_like(x0) for _ in range(S)]
        nxt = torch.empty_like(x0)
        bufs[0].copy_(x0)
        k = torch.empty((ops.RK_STAGES, *x0.shape), dtype=torch.float32, device=x.device)
        d = torch.zeros((ops.RK_STAGES, rows), dtype=torch.float64, device=x.device)
        delta = torch.zeros(rows, dtype=torch.float64, device=x.device)
        partials = torch.empty(ops.rk_partial_count(rows, n), dtype=torch.float64, device=x.device) if n > 1024 else None
        for h in tab.h:
            for i in range(S):
                out, g = _logp_network(model, bufs[i], times[e], eps, kwargs)
                last = i == S - 1
                if out.dtype != torch.float32:
                    out = out.to(torch.float32)
                ops.flow_logp_stage(i, out, g, eps, bufs[0], bufs[i] if i else None, coef, e, k, d, stage_coeffs(i), h,
                                    x_out=nxt if last else bufs[i + 1], delta=delta if last else None, partials=partials)
                e += 1
            bufs[0], nxt = nxt, bufs[0]
        z = bufs[0]
        prior = ops.flow_logp_prior(z, partials)
    else:
        # the same arithmetic as tensor operations: the table's float32 (A, B) for a float32 state, the float64 ones otherwise
        widen = (lambda v: float(np.float32(v))) if x.dtype == torch.float32 else float
        cur, delta = x0, torch.zeros(rows, dtype=torch.float64, device=x.device)
        for h in tab.h:
            ks, ds, xs = [], [], cur
            for i in range(S):
                out, g = _logp_network(model, xs.contiguous(), times[e], eps, kwargs)
                A, B = (widen(v) for v in tab.ab[e])
                ks.append(A * xs + B * out)
                ds.append(A * n + B * (eps.to(torch.float64) * g.to(torch.float64)).flatten(1).sum(1))
                xs = cur + h * _rk_combine(stage_coeffs(i), ks)
                e += 1
            delta = delta + h * _rk_combine(tab.b, ds)
            cur = xs
        z = cur
        prior = -0.5 * (z.to(torch.float64) ** 2).flatten(1).sum(1) - 0.5 * n * _LN_2PI
    delta_logp = delta.view(K, N).mean(0) if K > 1 else delta
    prior_logp, z = prior[:N], z[:N]
    logp = prior_logp + delta_logp
    return {"logp": logp, "prior_logp": prior_logp, "delta_logp": delta_logp, "bpd": -logp / (n * math.log(2.0)) + offset_bits,
            "z": z.clone() if use else z, "nfev": e, "nvjp": e}

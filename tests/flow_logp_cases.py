"""Support for the flow log-likelihood tests (no test in here): a float64 restatement of the augmented integration

    d/dt (x, l) = (v(x, t), div v(x, t)),   log p0(x0) = log N(x(t_hi); 0, I) + l(t_hi)

written independently of vaw_amd.samplers (its own tableaus, the divergence either exact or from fixed Hutchinson probes through
torch.autograd of the FIELD itself, the field from the reference's x0 / eps conversion and not from the collapsed A x + B out),
the stand-in models, and the case tables the CPU and GPU tests share."""
import math

import numpy as np
import torch

# c, a (strictly lower triangle), b of the explicit solvers
TABLEAUS = {"euler": ([0.0], [[]], [1.0]),
            "heun": ([0.0, 1.0], [[], [1.0]], [0.5, 0.5]),
            "rk4": ([0.0, 0.5, 0.5, 1.0], [[], [0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], [1 / 6, 1 / 3, 1 / 3, 1 / 6])}
MEAN_TYPES = ("START_X", "EPSILON", "VELOCITY", "VECTOR")
PATHS = ("linear", "cosine", "linear_logsnr")


def gaussian_logp(z):
    z = z.to(torch.float64).flatten(1)
    return -0.5 * (z ** 2).sum(1) - 0.5 * z.shape[1] * math.log(2 * math.pi)


def hutchinson_div(field, eps):
    """x, t -> (v, sum eps * (dv/dx)^T eps) per row, by one vector-Jacobian product through `field`."""
    def both(x, t):
        with torch.enable_grad():
            xr = x.detach().requires_grad_(True)
            v = field(xr, t)
            (g,) = torch.autograd.grad(v, xr, eps)
        return v.detach(), (eps * g).flatten(1).sum(1)
    return both


def integrate(field_div, x0, grid, solver):
    """The augmented system on `grid` (float64 numpy, ascending) from x0 (float64 [N, ...]).  field_div(x, t) -> (v, div) with
    t a Python float.  Returns {z, delta_logp, prior_logp, logp}."""
    c, a, b = TABLEAUS[solver]
    x, l = x0.to(torch.float64), torch.zeros(x0.shape[0], dtype=torch.float64)
    for k in range(len(grid) - 1):
        t0, t1 = float(grid[k]), float(grid[k + 1])
        h = t1 - t0
        ks, ds = [], []
        for i, ci in enumerate(c):
            xi = x
            for j, aij in enumerate(a[i]):
                if aij != 0:
                    xi = xi + h * aij * ks[j]
            v, dv = field_div(xi, t1 if ci == 1.0 else t0 + ci * h)
            ks.append(v)
            ds.append(dv)
        x = x + h * sum(bi * ki for bi, ki in zip(b, ks))
        l = l + h * sum(bi * di for bi, di in zip(b, ds))
    prior = gaussian_logp(x)
    return {"z": x, "delta_logp": l, "prior_logp": prior, "logp": prior + l}


# ---- the reference's conversion of a model output to the vector field (convert_model_output_to_vector), float64 ------------------
def reference_vector(interpolant, mean_type, out, x, t):
    """v from the model output through x0 / eps, as the reference forms it; t broadcastable against x."""
    a, s, da, ds = interpolant(t)
    if mean_type == "START_X":
        x0 = out
        eps = (x - a * x0) / s
    elif mean_type == "EPSILON":
        eps = out
        x0 = (x - s * eps) / a
    elif mean_type == "VELOCITY":
        den = a ** 2 + s ** 2
        x0, eps = (a * x - s * out) / den, (s * x + a * out) / den
    elif mean_type == "VECTOR":
        return out
    else:
        raise KeyError(mean_type)
    return da * x0 + ds * eps


def model_field(fm, model, **model_kwargs):
    """x, t (Python float) -> v of `model` under the flow object `fm` (anything with interpolant and model_mean_type)."""
    def field(x, t):
        tb = torch.full((x.shape[0],), t, dtype=x.dtype)
        out = model(x, tb, **model_kwargs)
        out = out[0] if isinstance(out, tuple) else out
        out = out[:, : x.shape[1]]
        return reference_vector(fm.interpolant, fm.model_mean_type.name, out, x, tb.view(-1, *([1] * (x.dim() - 1))))
    return field


def restate(fm, model, x0, probes, t_span, num_steps, solver, **model_kwargs):
    """flow_log_likelihood in float64: `probes` is [K, N, ...]; the divergence rows of the K probes are averaged."""
    grid = np.linspace(t_span[0], t_span[1], num_steps, dtype=np.float64)
    field = model_field(fm, model, **model_kwargs)
    runs = [integrate(hutchinson_div(field, e.to(torch.float64)), x0, grid, solver) for e in probes]
    delta = torch.stack([r["delta_logp"] for r in runs]).mean(0)
    return {"z": runs[0]["z"], "delta_logp": delta, "prior_logp": runs[0]["prior_logp"], "logp": runs[0]["prior_logp"] + delta}


# ---- stand-in models ---------------------------------------------------------------------------------------------------------
class Standin(torch.nn.Module):
    """A small smooth network in plain torch operations, any dtype and device: every output element depends on its neighbours
    along the last axis and on the other channels, so the Jacobian is full enough for a probe to matter.  sigma=True returns
    2C channels (a learn_sigma model's layout: the mean first)."""

    def __init__(self, channels, sigma=False, seed=5, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.mix = torch.nn.Parameter((torch.randn(channels, channels, generator=g, dtype=torch.float64) * 0.6).to(dtype), requires_grad=False)
        self.sigma = sigma

    def forward(self, x, t, **_):
        tb = t.view(-1, *([1] * (x.dim() - 1))).to(x.dtype)
        h = torch.einsum("dc,nc...->nd...", self.mix.to(x.dtype), x) + 0.5 * x.roll(1, -1) - 0.25 * x.roll(-1, -1)
        out = torch.tanh(h + tb) + 0.3 * x * tb
        return torch.cat((out, torch.sin(out)), 1) if self.sigma else out


# t_span per mean type and path that keeps the conversion regular: START_X divides by sigma (0 at t = 0), EPSILON by alpha
# (0 at t = 1 on the linear and cosine paths)
def regular_span(mean_type):
    return {"START_X": (0.1, 1.0), "EPSILON": (0.0, 0.9)}.get(mean_type, (0.0, 1.0))


# (rows, sample shape, learn_sigma): per-sample sizes 75 (off the vector width), 192 (one workgroup, vector), 4100 (five
# workgroups a row: the two-pass sum)
KERNEL_CASES = [(1, (3, 5, 5), False), (3, (3, 5, 5), False), (3, (3, 8, 8), False), (1, (4, 25, 41), False), (3, (4, 25, 41), False),
                (3, (3, 8, 8), True), (1, (3, 5, 5), True)]
SOLVERS = ("euler", "heun", "rk4")

"""Post-hoc EMA restated in float64 numpy for the tests of vaw_amd/ema.py: it imports nothing of the package's mathematics.

    sigma_rel^2 = (gamma + 1) / ((gamma + 2)^2 (gamma + 3))                 gamma: the largest real root of the cubic this gives
    p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t]      the continuous profile that ends at t
    update t = 1, 2, ...:  e <- e + (theta_t - e) c_t,  c_t = 1 - (1 - 1/t)^(gamma + 1)
    x = solve(A, b) / sum,  A_ij = <p_i, p_j>,  b_i = <p_i, p_out>           over the snapshots with t_i <= t_out
"""
import numpy as np
import torch
import torch.nn as nn


def gamma_of(sigma_rel):
    s = 1.0 / (sigma_rel * sigma_rel)
    roots = np.roots([1.0, 7.0, 16.0 - s, 12.0 - s])
    return float(np.max(roots[np.abs(roots.imag) < 1e-9].real))


def sigma_rel_of(gamma):
    return float(np.sqrt((gamma + 1) / ((gamma + 2) ** 2 * (gamma + 3))))


def profile(tau, t, gamma):
    return np.where(tau <= t, (gamma + 1) * (tau / t) ** gamma / t, 0.0)


def dot_quadrature(ta, ga, tb, gb, points):
    """midpoint rule over [0, min(ta, tb)], where both profiles live"""
    hi = min(ta, tb)
    h = hi / points
    total = 0.0
    for lo in range(0, points, 500_000):                      # in slabs: 3e6 points at once would be 100 MB of temporaries
        tau = (np.arange(lo, min(points, lo + 500_000), dtype=np.float64) + 0.5) * h
        total += float(np.sum(profile(tau, ta, ga) * profile(tau, tb, gb)))
    return total * h


def dot_closed(ta, ga, tb, gb):
    """the integral above by hand: int_0^ta tau^(ga+gb) dtau = ta^(ga+gb+1) / (ga+gb+1), for ta <= tb"""
    if ta > tb:
        ta, ga, tb, gb = tb, gb, ta, ga
    return (ga + 1) * (gb + 1) / (ga + gb + 1) * np.exp(gb * (np.log(ta) - np.log(tb))) / tb


def coef(t, gamma):
    return 1.0 if t == 1 else float(-np.expm1((gamma + 1) * np.log1p(-1.0 / t)))


def discrete_weights(T, gamma):
    """w[j-1]: the weight of theta_j in the tracked average after update T"""
    w = np.zeros(T, dtype=np.float64)
    for t in range(1, T + 1):
        c = coef(t, gamma)
        w *= 1.0 - c
        w[t - 1] += c
    return w


def track(theta, gamma, keep=()):
    """theta [T, W] -> (the average after update T, {t: the average after update t for t in keep})"""
    e = np.zeros(theta.shape[1], dtype=np.float64)
    kept = {}
    for t in range(1, theta.shape[0] + 1):
        e = e + (theta[t - 1] - e) * coef(t, gamma)
        if t in keep:
            kept[t] = e.copy()
    return e, kept


def solve(steps, gammas, t_out, g_out):
    """normalised least-squares weights of the snapshots (steps[i], gammas[i]), all of them at or before t_out"""
    n = len(steps)
    A = np.array([[dot_closed(steps[i], gammas[i], steps[j], gammas[j]) for j in range(n)] for i in range(n)])
    b = np.array([dot_closed(steps[i], gammas[i], t_out, g_out) for i in range(n)])
    x = np.linalg.lstsq(A, b, rcond=None)[0] if n > 1 else b / A[0]
    return x / x.sum(), A


def random_walk(T, width, seed=0):
    return np.cumsum(0.01 * np.random.default_rng(seed).standard_normal((T, width)), axis=0)


def walk_module(width, extra=0):
    """the smallest FlatModule: one trainable vector (and optionally a second, so that two modules differ in layout)"""
    import vaw_amd

    class Walk(vaw_amd.FlatModule):
        def __init__(self):
            super().__init__()
            self.theta = nn.Parameter(torch.zeros(width))
            if extra:
                self.more = nn.Parameter(torch.zeros(extra))

    return Walk()


def composition(e, p, c):
    """one tracked update as f32 tensor operations, each rounded on its own; c == 1 is the exact copy"""
    c = float(np.float32(c))
    return p.clone() if c == 1.0 else e.add((p - e).mul(c))

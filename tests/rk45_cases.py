"""Shared by test_rk45_cpu.py, test_gpu_rk45.py and tests/golden/make_rk45_goldens.py: the cases of tests/golden/rk45.npz
(adaptive Dormand-Prince 5(4) for the flow ODE, pinned against float64 scipy.integrate.solve_ivp(method="RK45")), their
stand-in network in float32 (torch) and float64 (numpy), and the drift the float64 oracle integrates."""
import numpy as np
import torch

RTOL, ATOL, SEED = 1e-4, 1e-5, 1          # not the default rtol = 1e-3: float32 and float64 take other accept / reject sequences there
PATHS = [("linear", "VELOCITY"), ("cosine", "VELOCITY"), ("linear", "VECTOR")]
SHAPES = [(3, 3, 5, 5), (2, 4, 8, 8)]          # 75 elements a row: scalar accesses; 256: 16-byte accesses
CASES = [(path, mean, shape) for path, mean in PATHS for shape in SHAPES]


def case_id(case):
    path, mean, shape = case
    return f"{path}-{mean}-{'x'.join(map(str, shape))}"


def standin(x, t, y=None, **kw):
    """0.6 tanh(2x) + 0.5 sin(12 t) + 0.02 y, t the flow time the model receives."""
    col = lambda v: v.reshape(-1, *([1] * (x.dim() - 1))).to(x.dtype)
    return 0.6 * torch.tanh(2 * x) + 0.5 * torch.sin(12 * col(t)) + 0.02 * col(y)


def inputs(shape, device="cpu"):
    """(x0, y) of a case: torch.manual_seed(SEED), randn(shape) on the CPU; y = arange(B) * 3 + 1."""
    torch.manual_seed(SEED)
    return torch.randn(shape).to(device), (torch.arange(shape[0]) * 3 + 1).to(device)


def drift64(path, mean, y_flat):
    """dx/dt (t, x) of the case in float64 numpy over the flattened batch: the stand-in through _flow_fields' conversion."""
    def f(t, x):
        out = 0.6 * np.tanh(2 * x) + 0.5 * np.sin(12 * t) + 0.02 * y_flat
        if mean == "VECTOR":
            return out
        if path == "linear":
            a, s, da, ds = 1 - t, t, -1.0, 1.0
        else:
            a, s = np.cos(t * np.pi / 2), np.sin(t * np.pi / 2)
            da, ds = -np.pi / 2 * s, np.pi / 2 * a
        den = a ** 2 + s ** 2
        return da * ((a * x - s * out) / den) + ds * ((s * x + a * out) / den)
    return f


def scipy_run(path, mean, x0, y):
    """float64 solve_ivp(RK45) from t = 1 to 0: (final state shaped like x0, nfev, attempts = (nfev - 2) / 6, accepted steps)."""
    from scipy.integrate import solve_ivp
    y_flat = np.repeat(y.double().numpy(), x0[0].numel())
    sol = solve_ivp(drift64(path, mean, y_flat), (1.0, 0.0), x0.double().numpy().ravel(), method="RK45", rtol=RTOL, atol=ATOL)
    assert sol.success and (sol.nfev - 2) % 6 == 0
    return sol.y[:, -1].reshape(x0.shape), int(sol.nfev), (int(sol.nfev) - 2) // 6, len(sol.t) - 1


def flow(path, mean, **extra):
    import vaw_amd
    from sampler_cases import sampler_args
    return vaw_amd.FlowMatching(args=sampler_args("flow", dict(guidance_scale=1.0), path_type=path, **extra),
                                model_mean_type=vaw_amd.ModelMeanType[mean])

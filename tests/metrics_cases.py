"""Shared by test_metrics_cpu.py and test_gpu_metrics.py: the seeded activation sets of the metric tests and a float64 numpy
restatement of ManifoldEstimator.manifold_radii / evaluate_pr and Evaluator.compute_statistics.  The restatement takes squared
distances directly as sum((u - v)^2), not through the norm expansion the kernels (and the reference) use, so it shares no
cancellation with the code under test.  Every reference is computed once per process and must not be modified."""
import functools

import numpy as np

RANK = 6
# (N1, N2, D, nhood_sizes, seed): off every tile edge (128 rows, 16 along D), odd D with unaligned rows, N1 != N2, two
# neighbourhood sizes.  The seeds are the smallest for which the float64 restatement alone meets test_metrics_cpu's conditions.
CASES = [
    (300, 260, 40, (3,), 4),
    (257, 130, 23, (3,), 6),
    (193, 200, 2023, (3,), 1),
    (130, 257, 2048, (3, 5), 14),
    (70, 70, 8, (5,), 1),
]
STATS_ONLY_CASE = (1, 3, 5, 0)          # for row_sqnorms and the statistics entry points only
CASE_IDS = [f"{a}x{b}x{d}" for a, b, d, _, _ in CASES]

TOL_D_FACTOR = 2e-6                     # tolD = 2e-6 * (max |u|^2 + max |v|^2): see test_gpu_metrics.py for the derivation


def make_features(n1, n2, d, seed):
    """Non-negative features of rank 6 plus a little full-rank noise, like ReLU activations: max(z P + off + 0.01 noise, 0).  The
    second ('sample') set draws z scaled by 0.8 and shifted by 0.5, so precision and recall land strictly between 0 and 1."""
    rng = np.random.default_rng(seed)
    proj = rng.standard_normal((RANK, d)) / np.sqrt(RANK)
    off = rng.uniform(0.5, 1.5, d)
    z1 = rng.standard_normal((n1, RANK))
    z2 = 0.8 * rng.standard_normal((n2, RANK)) + 0.5
    f1 = np.maximum(z1 @ proj + off + 0.01 * rng.standard_normal((n1, d)), 0).astype(np.float32)
    f2 = np.maximum(z2 @ proj + off + 0.01 * rng.standard_normal((n2, d)), 0).astype(np.float32)
    return f1, f2


def sqdist(u, v):
    """float64 [nu, nv]: sum_k (u_ik - v_jk)^2, taken directly."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    out = np.empty((len(u), len(v)))
    step = max(1, (1 << 24) // (len(v) * u.shape[1]))
    for i in range(0, len(u), step):
        out[i:i + step] = ((u[i:i + step, None, :] - v[None, :, :]) ** 2).sum(-1)
    return out


def tol_d(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return TOL_D_FACTOR * ((u * u).sum(1).max() + (v * v).sum(1).max())


def ref_sorted(x):
    """Every row's distances to all rows (itself included), ascending."""
    return np.sort(sqdist(x, x), axis=1)


def ref_radii(x, nhood_sizes):
    return ref_sorted(x)[:, list(nhood_sizes)]


def ref_flags(d, radii_1, radii_2):
    """DistanceBlock.less_thans on a whole distance matrix: (batch_1_in [N1, K2], batch_2_in [N2, K1])."""
    return (d[:, :, None] <= radii_2[None, :, :]).any(1), (d[:, :, None] <= radii_1[:, None, :]).any(0)


def ambiguous_flags(d, radii_1, radii_2, tol):
    """A flag is ambiguous when no pair decides it clearly (d <= r - 2 tol) and some pair lies within 2 tol of its radius."""
    def amb(lhs, axis):
        return ~(lhs <= -2 * tol).any(axis) & (np.abs(lhs) <= 2 * tol).any(axis)
    return amb(d[:, :, None] - radii_2[None, :, :], 1), amb(d[:, :, None] - radii_1[:, None, :], 0)


def ref_statistics(x):
    x = np.asarray(x, np.float64)
    return x.mean(0), np.cov(x, rowvar=False)


@functools.lru_cache(maxsize=None)
def reference(index):
    """Everything the tests need of CASES[index], in float64, computed once."""
    n1, n2, d, nhood, seed = CASES[index]
    f1, f2 = make_features(n1, n2, d, seed)
    s1, s2 = ref_sorted(f1), ref_sorted(f2)
    r1, r2 = s1[:, list(nhood)], s2[:, list(nhood)]
    d12 = sqdist(f1, f2)
    in1, in2 = ref_flags(d12, r1, r2)
    tol = max(tol_d(f1, f1), tol_d(f2, f2), tol_d(f1, f2))
    amb1, amb2 = ambiguous_flags(d12, r1, r2, tol)
    ref = dict(f1=f1, f2=f2, nhood=nhood, sorted1=s1, sorted2=s2, radii1=r1, radii2=r2, d12=d12, in1=in1, in2=in2, tol=tol,
               amb1=amb1, amb2=amb2, precision=in2.astype(np.float64).mean(0), recall=in1.astype(np.float64).mean(0))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def min_gap(sorted_d, count):
    """Smallest difference between neighbours among each row's first `count` sorted distances."""
    return float(np.diff(sorted_d[:, :count], axis=1).min())

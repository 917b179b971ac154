"""Shared by test_kid_dc_cpu.py and test_gpu_kid_dc.py: a float64 numpy restatement of the polynomial kernel matrices, the unbiased
MMD^2, the KID subset protocol (tests/golden/KID_DC.md) and the density / coverage counts and flags, on the seeded activation sets of
metrics_cases.py (nearest_k = 5) and on exact integer cases.  Distances come from metrics_cases.sqdist, compared with `<`.  Every
reference is computed once per process and must not be modified.

Tolerance of a kernel row sum.  The f32 MFMA chain of a dot product differs from the exact sum by at most MFMA_REL * A, A = sum_k
|u_k v_k| (3.5e-7 up to K = 4096: docstring of test_gpu_metrics.py).  k = (gamma dot + coef0)^degree has |dk / d dot| <= degree gamma
(gamma A + |coef0|)^(degree - 1) on the whole interval between the two dots, so an element moves by at most that times MFMA_REL A.
The float64 epilogue (the product gamma dot, the sum with coef0, degree - 1 products, nv sums) adds below (degree + 1 + nv) 1.2e-16
relative to sum_j |k_ij|; SUM_REL = 1e-12 covers it for every nv here.  A total over rows adds the row bounds and SUM_REL once more."""
import functools

import numpy as np

import metrics_cases as mc

NEAREST_K = 5
MFMA_REL = 3.5e-7
SUM_REL = 1e-12
DEGREE, COEF0 = 3, 1.0            # the KID kernel; gamma = 1 / D
CASE_IDS = mc.CASE_IDS


def kernel_matrix(u, v, gamma, coef0, degree):
    """float64 [nu, nv]: (gamma u_i . v_j + coef0)^degree."""
    t = gamma * (np.asarray(u, np.float64) @ np.asarray(v, np.float64).T) + coef0
    k = t.copy()
    for _ in range(degree - 1):
        k = k * t
    return k


def _keep(iu, iv, skip_diagonal):
    """[nu, nv] mask of the pairs that count: all, or those whose two source rows differ."""
    return np.ones((len(iu), len(iv)), bool) if not skip_diagonal else np.asarray(iu)[:, None] != np.asarray(iv)[None, :]


def row_sums(u, v, gamma, coef0, degree, skip_diagonal=False, iu=None, iv=None):
    """float64 [nu]: sum_j k(u_i, v_j) over the kept pairs; iu / iv are the source rows (default: the positions)."""
    iu, iv = (np.arange(len(u)) if iu is None else iu), (np.arange(len(v)) if iv is None else iv)
    return np.where(_keep(iu, iv, skip_diagonal), kernel_matrix(u, v, gamma, coef0, degree), 0.0).sum(1)


def row_sum_bound(u, v, gamma, coef0, degree, skip_diagonal=False, iu=None, iv=None):
    """float64 [nu]: the tolerance of a kernel row sum derived in the module docstring."""
    iu, iv = (np.arange(len(u)) if iu is None else iu), (np.arange(len(v)) if iv is None else iv)
    a = np.abs(np.asarray(u, np.float64)) @ np.abs(np.asarray(v, np.float64)).T
    per_pair = degree * abs(gamma) * (abs(gamma) * a + abs(coef0)) ** (degree - 1) * MFMA_REL * a
    keep = _keep(iu, iv, skip_diagonal)
    return np.where(keep, per_pair, 0.0).sum(1) + SUM_REL * np.where(keep, np.abs(kernel_matrix(u, v, gamma, coef0, degree)), 0.0).sum(1)


def mmd2(x, y, gamma, coef0, degree, variant="unbiased"):
    """The unbiased estimator, or a wrong variant the tolerance must tell apart: 'diagonal' keeps the i == j terms under the unbiased
    denominators, 'biased' divides the i != j sums by m^2 and n^2."""
    m, n = len(x), len(y)
    skip = variant != "diagonal"
    sxx = row_sums(x, x, gamma, coef0, degree, skip).sum()
    syy = row_sums(y, y, gamma, coef0, degree, skip).sum()
    sxy = row_sums(x, y, gamma, coef0, degree).sum()
    dx, dy = (m * m, n * n) if variant == "biased" else (m * (m - 1), n * (n - 1))
    return sxx / dx + syy / dy - 2 * sxy / (m * n)


def mmd2_bound(x, y, gamma, coef0, degree):
    """The row-sum tolerances carried through the estimator, and SUM_REL of every total for its summation over rows."""
    m, n = len(x), len(y)
    out = 0.0
    for u, v, skip, den in ((x, x, True, m * (m - 1)), (y, y, True, n * (n - 1)), (x, y, False, m * n / 2)):
        out += (row_sum_bound(u, v, gamma, coef0, degree, skip).sum() + SUM_REL * np.abs(row_sums(u, v, gamma, coef0, degree, skip)).sum()) / den
    return out


def subset_indices(n_ref, n_sample, num_subsets, subset_size, seed):
    """tests/golden/KID_DC.md: one RandomState(seed); per subset a draw without replacement from the reference set, then one from the
    sample set."""
    rng = np.random.RandomState(seed)
    pairs = [(rng.choice(n_ref, subset_size, replace=False), rng.choice(n_sample, subset_size, replace=False)) for _ in range(num_subsets)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def kid_scores(ref, sample, num_subsets, subset_size, seed, gamma, coef0=COEF0, degree=DEGREE):
    """(scores, bounds), float64 [num_subsets]: the unbiased MMD^2 of every subset pair and its tolerance."""
    ri, si = subset_indices(len(ref), len(sample), num_subsets, subset_size, seed)
    scores = np.array([mmd2(ref[a], sample[b], gamma, coef0, degree) for a, b in zip(ri, si)])
    bounds = np.array([mmd2_bound(ref[a], sample[b], gamma, coef0, degree) for a, b in zip(ri, si)])
    return scores, bounds


def counts_and_flags(d, radii, strict=True):
    """d [M, N] generated x real, radii [N, K] of the real points: (counts int64 [M, K], flags bool [N, K])."""
    under = d[:, :, None] < radii[None, :, :] if strict else d[:, :, None] <= radii[None, :, :]
    return under.sum(1), under.any(0)


def density_coverage(counts, flags, nhood_sizes):
    return counts.sum(0) / (np.asarray(nhood_sizes, np.float64) * len(counts)), flags.astype(np.float64).mean(0)


def _freeze(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(index):
    """CASES[index] of metrics_cases: set 1 is the reference ('real') set, set 2 the sample ('generated') set."""
    r = mc.reference(index)
    f1, f2, tol = r["f1"], r["f2"], r["tol"]
    gamma = 1.0 / f1.shape[1]
    radii = r["sorted1"][:, [NEAREST_K]]
    d = np.ascontiguousarray(r["d12"].T)                                    # generated x real
    counts, flags = counts_and_flags(d, radii)
    lo, decided = counts_and_flags(d, radii - 2 * tol)
    hi, _ = counts_and_flags(d, radii + 2 * tol)
    near = np.abs(d[:, :, None] - radii[None, :, :]) <= 2 * tol
    density, coverage = density_coverage(counts, flags, (NEAREST_K,))
    out = dict(f1=f1, f2=f2, gamma=gamma, tol=tol, radii=radii, d=d, counts=counts, flags=flags, counts_lo=lo, counts_hi=hi,
               ambiguous_rows=near.any((1, 2)), ambiguous_flags=~decided & near.any(0), near_pairs=int(near.sum()),
               density=density, coverage=coverage, mmd2=mmd2(f1, f2, gamma, COEF0, DEGREE), mmd2_bound=mmd2_bound(f1, f2, gamma, COEF0, DEGREE))
    for name, u, v in (("11", f1, f1), ("22", f2, f2), ("12", f1, f2)):
        for skip in (False, True) if u is v else (False,):
            key = name + ("_skip" if skip else "")
            out["rows_" + key] = row_sums(u, v, gamma, COEF0, DEGREE, skip)
            out["bound_" + key] = row_sum_bound(u, v, gamma, COEF0, DEGREE, skip)
    return _freeze(out)


# (N real, N generated, D, seed): integer features 0 .. 3 with gamma = 1/16 and coef0 = 1.  Every dot product is an integer below
# 2^8, every kernel value (16 + dot)^3 / 2^12 and every sum of them is exact in float64, every square distance an integer exact in
# f32.  Off the 128-row tile edge, D on and off the 16-wide slab.
EXACT_CASES = [(150, 140, 16, 21), (131, 150, 23, 22)]
EXACT_IDS = [f"{a}x{b}x{d}" for a, b, d, _ in EXACT_CASES]
EXACT_GAMMA = 1.0 / 16


@functools.lru_cache(maxsize=None)
def exact_reference(index):
    """Integer sets with rows copied between them (d == 0) -- among them, for real points 0 .. 19, the very neighbour that sets
    the point's radius, so the generated copy lies exactly on that radius (d == r): `<` leaves it out, `<=` would count it."""
    n1, n2, dim, seed = EXACT_CASES[index]
    rng = np.random.default_rng(seed)
    real = rng.integers(0, 4, (n1, dim)).astype(np.float32)
    fake = rng.integers(0, 4, (n2, dim)).astype(np.float32)
    d11 = mc.sqdist(real, real)
    order = np.argsort(d11, axis=1, kind="stable")
    radii = np.sort(d11, axis=1)[:, [NEAREST_K]]
    fake[:20] = real[order[:20, NEAREST_K]]                                 # at distance exactly radii[j] from real point j
    fake[20:30] = real[40:50]
    d = mc.sqdist(fake, real)
    counts, flags = counts_and_flags(d, radii)
    counts_le, flags_le = counts_and_flags(d, radii, strict=False)
    density, coverage = density_coverage(counts, flags, (NEAREST_K,))
    out = dict(real=real, fake=fake, radii=radii, d=d, counts=counts, flags=flags, counts_le=counts_le, flags_le=flags_le, density=density,
               coverage=coverage, ties=int((d[:, :, None] == radii[None, :, :]).sum()), zeros=int((d == 0).sum()),
               mmd2=mmd2(real, fake, EXACT_GAMMA, COEF0, DEGREE))
    for name, u, v in (("11", real, real), ("22", fake, fake), ("12", real, fake)):
        for skip in (False, True) if u is v else (False,):
            out["rows_" + name + ("_skip" if skip else "")] = row_sums(u, v, EXACT_GAMMA, COEF0, DEGREE, skip)
    return _freeze(out)

"""The polynomial-kernel row sums and the counts under radii (csrc/metrics.hip), and KID / density / coverage of vaw_amd.evaluator,
on the GPU against the float64 restatement of kid_dc_cases.py.  Run on the MI355X box: pytest -m gpu tests/test_gpu_kid_dc.py.

The tolerance of a row sum is derived in kid_dc_cases.py from the f32 MFMA chain's bound (3.5e-7 sum |u v|) carried through the
derivative of the kernel; tolD of the distances is test_gpu_metrics.py's.  Both come from the number formats, not from what the
kernels were seen to give; every test prints its measured figure before it asserts."""
import numpy as np
import pytest
import torch

import kid_dc_cases as kc
import metrics_cases as mc

pytestmark = pytest.mark.gpu

from vaw_amd import evaluator as ev, ops

DEV = "cuda"
CASE_IDX = range(len(mc.CASES))
EXACT_IDX = range(len(kc.EXACT_CASES))


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)      # a copy: the shared references are read-only arrays


def _np(t):
    return t.cpu().numpy()


def _polysum(u, v, gamma, skip=False, u_idx=None, v_idx=None):
    return _np(ops.pairwise_polysum(u, v, gamma, kc.COEF0, kc.DEGREE, u_idx=u_idx, v_idx=v_idx, skip_diagonal=skip))


@pytest.mark.parametrize("index", CASE_IDX, ids=kc.CASE_IDS)
def test_row_sums_against_float64(index):
    r = kc.reference(index)
    f1, f2 = _dev(r["f1"]), _dev(r["f2"])
    for key, u, v, skip in (("11", f1, f1, False), ("11_skip", f1, f1, True), ("22", f2, f2, False), ("22_skip", f2, f2, True),
                            ("12", f1, f2, False)):
        got = _polysum(u, v, r["gamma"], skip)
        assert got.shape == (1, len(u)) and got.dtype == np.float64
        ratio = np.abs(got[0] - r["rows_" + key]) / r["bound_" + key]
        print(f"[polysum {kc.CASE_IDS[index]} {key}] max |got - ref| / bound = {ratio.max():.4f}")
        assert np.all(ratio <= 1)
        assert np.array_equal(got, _polysum(u, v, r["gamma"], skip))                       # a second launch: the same bits


@pytest.mark.parametrize("index", [0, 3], ids=[kc.CASE_IDS[0], kc.CASE_IDS[3]])
def test_index_tables_against_gathered_rows_and_batches_alone(index):
    """Rows read through a table give the bits of rows gathered beforehand (with the diagonal taken from the table's values, which
    for a gathered set are its positions), and a batch alone the bits it has inside a 3-batch launch."""
    r = kc.reference(index)
    f1, f2, gamma = _dev(r["f1"]), _dev(r["f2"]), r["gamma"]
    size = 129 if min(len(f1), len(f2)) >= 129 else 64
    ri, si = kc.subset_indices(len(f1), len(f2), 3, size, 11)
    both = _polysum(f1, f2, gamma, False, ri, si)
    same = _polysum(f1, f1, gamma, True, ri, ri)
    half = _polysum(f1, f2, gamma, False, ri, None)                                         # one table only: all of f2, in order
    assert both.shape == same.shape == half.shape == (3, size)
    for b in range(3):
        u, v = f1[torch.from_numpy(ri[b]).to(DEV)].contiguous(), f2[torch.from_numpy(si[b]).to(DEV)].contiguous()
        assert np.array_equal(both[b], _polysum(u, v, gamma)[0])
        assert np.array_equal(same[b], _polysum(u, u, gamma, True)[0])
        assert np.array_equal(half[b], _polysum(u, f2, gamma)[0])
        assert np.array_equal(both[b], _polysum(f1, f2, gamma, False, ri[b:b + 1], si[b:b + 1])[0])
        assert np.array_equal(same[b], _polysum(f1, f1, gamma, True, ri[b:b + 1], ri[b:b + 1])[0])
        ref = kc.row_sums(r["f1"][ri[b]], r["f1"][ri[b]], gamma, kc.COEF0, kc.DEGREE, True)
        assert np.all(np.abs(same[b] - ref) <= kc.row_sum_bound(r["f1"][ri[b]], r["f1"][ri[b]], gamma, kc.COEF0, kc.DEGREE, True))
    with pytest.raises(ValueError, match="outside the rows"):
        _polysum(f1, f2, gamma, False, ri, si + len(f2))
    with pytest.raises(ValueError, match="outside the rows"):
        _polysum(f1, f2, gamma, False, -ri, si)
    with pytest.raises(ValueError, match="batches"):
        _polysum(f1, f2, gamma, False, ri, si[:2])


@pytest.mark.parametrize("degree", [1, 2, 8])
def test_every_degree_and_negative_parameters(degree):
    r = kc.reference(1)
    gamma, coef0 = -0.03, -0.5
    got = _np(ops.pairwise_polysum(_dev(r["f1"]), _dev(r["f2"]), gamma, coef0, degree))[0]
    ref = kc.row_sums(r["f1"], r["f2"], gamma, coef0, degree)
    bound = kc.row_sum_bound(r["f1"], r["f2"], gamma, coef0, degree)
    print(f"[polysum degree {degree}] max |got - ref| / bound = {np.max(np.abs(got - ref) / bound):.4f}")
    assert np.all(np.abs(got - ref) <= bound)


@pytest.mark.parametrize("index", EXACT_IDX, ids=kc.EXACT_IDS)
def test_exact_cases_equal_the_integer_restatement(index):
    """Integer features: row sums, the MMD^2, counts, flags, density and coverage are the restatement's, bit for bit; a generated
    point exactly on a radius (d == r) is not counted, a copied one (d == 0) is."""
    r = kc.exact_reference(index)
    real, fake = _dev(r["real"]), _dev(r["fake"])
    for key, u, v, skip in (("11", real, real, False), ("11_skip", real, real, True), ("22", fake, fake, False),
                            ("22_skip", fake, fake, True), ("12", real, fake, False)):
        assert np.array_equal(_polysum(u, v, kc.EXACT_GAMMA, skip)[0], r["rows_" + key]), key
    got = ev.polynomial_mmd2(r["real"], r["fake"], gamma=kc.EXACT_GAMMA)
    print(f"[exact {kc.EXACT_IDS[index]}] mmd2 {got!r} restatement {r['mmd2']!r}; {r['ties']} ties, {r['zeros']} zero distances")
    assert isinstance(got, float) and got == r["mmd2"]
    radii = _dev(r["radii"].astype(np.float32))
    counts = torch.zeros(len(fake), 1, device=DEV, dtype=torch.int32)
    flags = torch.zeros(len(real), 1, device=DEV, dtype=torch.uint8)
    ops.pairwise_count_within(fake, real, ops.row_sqnorms(fake), ops.row_sqnorms(real), radii, counts, flags)
    assert np.array_equal(_np(counts), r["counts"]) and np.array_equal(_np(flags).astype(bool), r["flags"])
    assert not np.array_equal(r["counts"], r["counts_le"])                                  # `<=` would have counted the ties
    est = ev.ManifoldEstimator(nhood_sizes=(kc.NEAREST_K,))
    assert np.array_equal(est.manifold_radii(r["real"]), r["radii"].astype(np.float32))
    density, coverage = est.evaluate_dc(r["real"], r["radii"], r["fake"])
    assert density.dtype == np.float64 and np.array_equal(density, r["density"]) and np.array_equal(coverage, r["coverage"])
    assert np.array_equal(est.last_counts, r["counts"]) and np.array_equal(est.last_covered, r["flags"])
    assert ev.compute_density_coverage(r["real"], r["fake"]) == (float(r["density"][0]), float(r["coverage"][0]))


def test_mmd2_of_the_full_sets_and_row_chunks(monkeypatch):
    for index in CASE_IDX:
        r = kc.reference(index)
        got = ev.polynomial_mmd2(r["f1"], r["f2"])
        print(f"[mmd2 {kc.CASE_IDS[index]}] got {got:.9f} ref {r['mmd2']:.9f}: |got - ref| / bound = {abs(got - r['mmd2']) / r['mmd2_bound']:.4f}")
        assert abs(got - r["mmd2"]) <= r["mmd2_bound"]
        if index < 2:                                          # cut into launches of 100 rows: a row's sum keeps its order
            monkeypatch.setattr(ev, "POLYSUM_MAX_ROWS", 100)
            assert ev.polynomial_mmd2(_dev(r["f1"]), _dev(r["f2"])) == got
            monkeypatch.undo()


@pytest.mark.parametrize("index,size", [(0, 64), (1, 129), (2, 64), (3, 129)])
def test_kid_against_float64(index, size, monkeypatch):
    """Four subsets of 64 rows, and of 129 (one row past a tile).  |std(a) - std(b)| <= max |a - b| and the same for the mean."""
    r = kc.reference(index)
    ref, bounds = kc.kid_scores(r["f1"], r["f2"], 4, size, 3, r["gamma"])
    got = ev.kid_subset_scores(r["f1"], r["f2"], num_subsets=4, subset_size=size, seed=3)
    print(f"[kid {kc.CASE_IDS[index]} subsets of {size}] scores {got}; max |got - ref| / bound = {np.max(np.abs(got - ref) / bounds):.4f}")
    assert got.dtype == np.float64 and got.shape == (4,) and np.all(np.abs(got - ref) <= bounds)
    mean, std = ev.compute_kid(_dev(r["f1"]), _dev(r["f2"]), num_subsets=4, subset_size=size, seed=3)
    assert (mean, std) == (float(np.mean(got)), float(np.std(got))) and isinstance(mean, float)
    assert abs(mean - ref.mean()) <= bounds.max() and abs(std - ref.std()) <= bounds.max()
    assert ev.Evaluator().compute_kid(r["f1"], r["f2"], num_subsets=4, subset_size=size, seed=3) == (mean, std)
    monkeypatch.setattr(ev, "KID_WORKSPACE_BYTES", 1)          # one subset per launch: the bits of the batched launches
    assert np.array_equal(ev.kid_subset_scores(r["f1"], r["f2"], num_subsets=4, subset_size=size, seed=3), got)
    assert not np.array_equal(ev.kid_subset_scores(r["f1"], r["f2"], num_subsets=4, subset_size=size, seed=4), got)


@pytest.mark.parametrize("index", CASE_IDX, ids=kc.CASE_IDS)
def test_density_coverage_against_float64(index):
    """Counts on the kernels' own radii: a pair counts in the restatement at r - 2 tolD => it counts here => it counts in the
    restatement at r + 2 tolD (a distance and a radius each move by at most tolD).  test_kid_dc_cpu shows that no flag is ambiguous."""
    r = kc.reference(index)
    out = []
    for rb, cb in ((10000, 10000), (64, 100)):
        est = ev.ManifoldEstimator(row_batch_size=rb, col_batch_size=cb, nhood_sizes=(kc.NEAREST_K,))
        density, coverage = est.evaluate_dc(r["f1"], est.manifold_radii(r["f1"]), r["f2"])
        out.append((est.last_counts, est.last_covered, density, coverage))
    counts, covered, density, coverage = out[0]
    loose = int((r["counts_lo"] != r["counts_hi"]).sum())
    print(f"[dc {kc.CASE_IDS[index]}] density {density} coverage {coverage}; restatement {r['density']} {r['coverage']}; "
          f"{loose} counts with a pair inside the band, {int((counts != r['counts']).sum())} differ from the restatement")
    assert counts.dtype == np.int32 and counts.shape == r["counts"].shape and covered.shape == r["flags"].shape
    assert np.all(r["counts_lo"] <= counts) and np.all(counts <= r["counts_hi"])
    assert np.array_equal(covered, r["flags"]) and np.array_equal(coverage, r["coverage"])
    assert density.dtype == np.float64 and density[0] == counts.sum(dtype=np.int64) / (kc.NEAREST_K * len(r["f2"]))
    for a, b in zip(out[0], out[1]):                           # no chunking shows in a count, a flag or a result
        assert a.dtype == b.dtype and np.array_equal(a, b)
    d, c = ev.compute_density_coverage(r["f1"], _dev(r["f2"]), manifold_estimator=ev.ManifoldEstimator(64, 100))
    assert isinstance(d, float) and (d, c) == (float(density[0]), float(coverage[0]))
    assert ev.Evaluator().compute_density_coverage(r["f1"], r["f2"], nearest_k=kc.NEAREST_K) == (d, c)


def test_two_neighbourhood_sizes_and_padding():
    """K = 2 radii per point in one pass equal two passes of one, and the padding of a mostly empty tile (21 x 19 rows) is under no
    radius, however large."""
    r = kc.reference(0)
    est = ev.ManifoldEstimator(nhood_sizes=(3, 5))
    radii = est.manifold_radii(r["f1"])
    density, coverage = est.evaluate_dc(r["f1"], radii, r["f2"])
    counts = est.last_counts
    for c, k in enumerate((3, 5)):
        one = ev.ManifoldEstimator(nhood_sizes=(k,))
        dk, ck = one.evaluate_dc(r["f1"], radii[:, [c]], r["f2"])
        assert np.array_equal(one.last_counts[:, 0], counts[:, c]) and dk[0] == density[c] and ck[0] == coverage[c]
    small = ev.ManifoldEstimator(nhood_sizes=(1,))
    d, c = small.evaluate_dc(r["f1"][:21], np.full((21, 1), 1e30, np.float32), r["f2"][:19])
    assert np.array_equal(small.last_counts, np.full((19, 1), 21)) and d[0] == 21.0 and c[0] == 1.0


def test_non_finite_features_are_refused():
    f = mc.reference(4)["f1"].copy()
    g = f.copy()
    g[17, 3] = np.nan
    for call in (lambda: ev.polynomial_mmd2(f, g), lambda: ev.compute_kid(g, f, num_subsets=2, subset_size=8),
                 lambda: ev.compute_density_coverage(f, g), lambda: ev.ManifoldEstimator().evaluate_dc(f, np.ones((70, 1)), g)):
        with pytest.raises(ValueError, match="NaN or inf"):
            call()


def test_metrics_from_activations_with_the_new_options():
    r = mc.reference(0)
    sp1, sp2 = mc.make_features(300, 260, 23, 9)
    plain = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2))
    assert set(plain) == {"fid", "sfid", "precision", "recall"}
    kid = dict(num_subsets=4, subset_size=64, seed=3)
    m = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2), kid=kid, density_coverage=True)
    assert set(m) == set(plain) | {"kid", "kid_std", "density", "coverage"} and all(isinstance(v, float) for v in m.values())
    assert {k: m[k] for k in plain} == plain
    assert (m["kid"], m["kid_std"]) == ev.compute_kid(r["f1"], r["f2"], **kid)
    assert (m["density"], m["coverage"]) == ev.compute_density_coverage(r["f1"], r["f2"], nearest_k=5)
    m3 = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2), density_coverage=3)
    assert set(m3) == set(plain) | {"density", "coverage"}
    assert (m3["density"], m3["coverage"]) == ev.compute_density_coverage(r["f1"], r["f2"], nearest_k=3)

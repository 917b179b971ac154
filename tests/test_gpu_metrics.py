"""The evaluation-metric kernels (csrc/metrics.hip) and vaw_amd.evaluator on the GPU against the float64 restatement of
metrics_cases.py.  Run on the MI355X box: pytest -m gpu tests/test_gpu_metrics.py.

Distance tolerance.  tolD = 2e-6 * (max |u|^2 + max |v|^2).  An f32 MFMA chain of length K differs from the exact sum by at most
3.5e-7 * sum |a b| up to K = 4096 (1.5e-7 up to K = 1024).  A distance is made of three such sums -- the two square norms and twice
the dot product, and sum |u v| <= (|u|^2 + |v|^2) / 2 -- so their errors add up to at most 7e-7 * (|u|^2 + |v|^2); the factor 2e-6 is
that with about 3x margin for the three roundings of the epilogue.  The bound comes from the number format, not from what the
kernels were seen to give; every test prints its measured figure before it asserts."""
import numpy as np
import pytest
import torch

import metrics_cases as mc

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import evaluator as ev, ops

DEV = "cuda"
EPS64 = 2.2e-16
CASE_IDX = range(len(mc.CASES))


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)      # a copy: the shared references are read-only arrays


def _np(t):
    return t.cpu().numpy()


def _ulp_bound(d, terms):
    """`terms` roundings of values no larger than d in f32."""
    return terms * 2.0 ** -24 * d


@pytest.mark.parametrize("shape", [(1, 5), (3, 5), (257, 23), (193, 2023), (130, 2048), (300, 40)])
def test_row_sqnorms(shape):
    n, d = shape
    x = mc.make_features(n, 2, d, 3)[0]
    got = _np(ops.row_sqnorms(_dev(x))).astype(np.float64)
    ref = (x.astype(np.float64) ** 2).sum(1)
    bound = (d / 64 + 8) * 2.0 ** -24 * ref          # one rounding per product, then sums (D / 64 + 6) deep
    print(f"[row_sqnorms {shape}] max err / bound = {np.max(np.abs(got - ref) / bound):.3f}")
    assert np.all(np.abs(got - ref) <= bound)
    assert np.array_equal(got, _np(ops.row_sqnorms(_dev(x))))


@pytest.mark.parametrize("index", CASE_IDX, ids=mc.CASE_IDS)
def test_ksmallest_and_radii_against_float64(index):
    """The k1 smallest distances of every row, ascending, within tolD of the sorted float64 distances (an order statistic moves by no
    more than the largest change of any one value), for a set against itself and for set 1 against set 2; manifold_radii takes its
    columns."""
    r = mc.reference(index)
    k1 = max(r["nhood"]) + 1
    for name, u, v, ref in (("1x1", r["f1"], r["f1"], r["sorted1"]), ("2x2", r["f2"], r["f2"], r["sorted2"]),
                            ("1x2", r["f1"], r["f2"], np.sort(r["d12"], axis=1))):
        got = _np(ops.pairwise_ksmallest(_dev(u), _dev(v), k1))
        tol = mc.tol_d(u, v)
        err = float(np.abs(got - ref[:, :k1]).max())
        print(f"[ksmallest {mc.CASE_IDS[index]} {name}] max |got - ref| = {err:.3e} = {err / tol:.4f} tolD")
        assert got.shape == (len(u), k1) and got.dtype == np.float32 and np.all(np.isfinite(got))
        assert np.all(np.diff(got, axis=1) >= 0) and np.all(got >= 0)
        assert err <= tol
    est = ev.ManifoldEstimator(nhood_sizes=r["nhood"])
    for f, ref in ((r["f1"], r["radii1"]), (r["f2"], r["radii2"])):
        radii = est.manifold_radii(f)
        assert radii.dtype == np.float32 and radii.shape == ref.shape
        assert np.abs(radii - ref).max() <= mc.tol_d(f, f)


def test_ksmallest_all_k1_and_device_inputs():
    """k1 = 1 .. 16 (three register-list widths) give prefixes of one another bit for bit; a device tensor is used in place and gives
    the bits of the numpy input."""
    r = mc.reference(0)
    u, v = _dev(r["f1"]), _dev(r["f2"])
    full = _np(ops.pairwise_ksmallest(u, v, 16))
    assert np.abs(full - np.sort(r["d12"], axis=1)[:, :16]).max() <= mc.tol_d(r["f1"], r["f2"])
    for k1 in (1, 2, 4, 5, 8, 9, 15):
        assert np.array_equal(_np(ops.pairwise_ksmallest(u, v, k1)), full[:, :k1]), k1
    est = ev.ManifoldEstimator()
    assert np.array_equal(est.manifold_radii(u), est.manifold_radii(r["f1"]))
    assert np.array_equal(est.manifold_radii(torch.from_numpy(r["f1"].astype(np.float64))), est.manifold_radii(r["f1"]))


def test_distance_symmetry():
    """(U, V) against (V, U) through k1 = nv calls, which return every distance of a row.  The dot product is the same fma chain
    either way, so with the two norm vectors equal to one constant the distances are equal bit for bit.  With the real norms the
    fixed order (norm_u - 2 dot) + norm_v rounds norm_u - 2 dot on one side and norm_v - 2 dot on the other: the two results are
    roundings of one exact value and differ by at most two roundings of a value below norm_u + norm_v, which is asserted instead."""
    r = mc.reference(4)
    u, v = _dev(r["f1"][:16]), _dev(r["f2"][:13])
    c16, c13 = torch.full((16,), 64.0, device=DEV), torch.full((13,), 64.0, device=DEV)
    uv = np.sort(_np(ops.pairwise_ksmallest(u, v, 13, c16, c13)), axis=None)
    vu = np.sort(_np(ops.pairwise_ksmallest(v, u, 16, c13, c16)), axis=None)
    assert uv.size == vu.size == 16 * 13 and np.array_equal(uv, vu) and np.unique(uv).size > 100
    uv = np.sort(_np(ops.pairwise_ksmallest(u, v, 13)), axis=None)
    vu = np.sort(_np(ops.pairwise_ksmallest(v, u, 16)), axis=None)
    bound = _ulp_bound(float(ops.row_sqnorms(u).max() + ops.row_sqnorms(v).max()), 2)
    print(f"[symmetry] real norms: max |d(U,V) - d(V,U)| = {np.abs(uv - vu).max():.3e}, bound {bound:.3e}")
    assert np.abs(uv - vu).max() <= bound


def _flags(u, v, radii_u, radii_v):
    u, v = _dev(u), _dev(v)
    ru, rv = _dev(radii_u.astype(np.float32)), _dev(radii_v.astype(np.float32))
    u_in = torch.zeros(len(u), rv.shape[1], device=DEV, dtype=torch.uint8)
    v_in = torch.zeros(len(v), ru.shape[1], device=DEV, dtype=torch.uint8)
    ops.pairwise_within(u, v, ops.row_sqnorms(u), ops.row_sqnorms(v), ru, rv, u_in, v_in)
    return _np(u_in), _np(v_in)


@pytest.mark.parametrize("index", CASE_IDX, ids=mc.CASE_IDS)
def test_flags_and_precision_recall_against_float64(index):
    """pairwise_within on the restatement's radii, and evaluate_pr / compute_prec_recall on the kernels' own radii.  Ambiguous flags
    are excluded and capped at 1 % of the flags; test_metrics_cpu shows that there are none on these seeds, so every flag matches and
    precision / recall are the restatement's exactly."""
    r = mc.reference(index)
    share = (r["amb1"].sum() + r["amb2"].sum()) / (r["amb1"].size + r["amb2"].size)
    assert share <= 0.01
    u_in, v_in = _flags(r["f1"], r["f2"], r["radii1"], r["radii2"])
    assert set(np.unique(u_in)) <= {0, 1} and set(np.unique(v_in)) <= {0, 1}
    bad = int(((u_in.astype(bool) != r["in1"]) & ~r["amb1"]).sum() + ((v_in.astype(bool) != r["in2"]) & ~r["amb2"]).sum())
    print(f"[flags {mc.CASE_IDS[index]}] ambiguous share {share:.4f}, mismatching decided flags {bad}")
    assert bad == 0
    est = ev.ManifoldEstimator(nhood_sizes=r["nhood"])
    precision, recall = est.evaluate_pr(r["f1"], est.manifold_radii(r["f1"]), r["f2"], est.manifold_radii(r["f2"]))
    print(f"[evaluate_pr {mc.CASE_IDS[index]}] precision {precision} recall {recall}; restatement {r['precision']} {r['recall']}")
    assert precision.dtype == np.float64 and precision.shape == (len(r["nhood"]),) and recall.shape == (len(r["nhood"]),)
    assert share > 0 or (np.array_equal(precision, r["precision"]) and np.array_equal(recall, r["recall"]))
    if len(r["nhood"]) == 1:
        p, q = ev.compute_prec_recall(r["f1"], r["f2"], ev.ManifoldEstimator(nhood_sizes=r["nhood"]))
        assert isinstance(p, float) and (p, q) == (float(precision[0]), float(recall[0]))


def _orthogonal_near_origin(n, d, seed):
    """n <= d points, one per axis, with norms from 1 to 2: any two are further apart (|x|^2 + |y|^2) than either is from the origin
    (|x|^2), so an unmasked zero row of the padding would be every point's nearest neighbour."""
    assert n <= d
    rng = np.random.default_rng(seed)
    x = 0.001 * rng.random((n, d))
    x[np.arange(n), np.arange(n) % d] += 1 + np.arange(n) / n
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", ["far", "near"])
def test_padding_never_wins(kind):
    """70 / 66 and 21 / 19 rows in 128-row tiles, 40 and 23 columns in slabs of 16: most of every tile is zero padding.  'far':
    all-positive features far from the origin, where the zero row is nearer to nothing (the mask must still keep its flags out);
    'near': features whose neighbours are all further away than the origin, where an unmasked zero row would be every point's
    nearest neighbour."""
    if kind == "far":
        rng = np.random.default_rng(9)                         # the smallest seed from 5 on with no ambiguous flag in float64
        f1, f2 = (10 + rng.random((70, 40))).astype(np.float32), (10 + 1.2 * rng.random((66, 40))).astype(np.float32)
    else:
        f1, f2 = _orthogonal_near_origin(21, 23, 1), _orthogonal_near_origin(19, 23, 2)
    est = ev.ManifoldEstimator()
    s1, s2, d12 = mc.ref_sorted(f1), mc.ref_sorted(f2), mc.sqdist(f1, f2)
    r1, r2 = est.manifold_radii(f1), est.manifold_radii(f2)
    tol = max(mc.tol_d(f1, f1), mc.tol_d(f2, f2))
    print(f"[padding {kind}] radii err {np.abs(r1 - s1[:, [3]]).max():.3e} {np.abs(r2 - s2[:, [3]]).max():.3e}, tolD {tol:.3e}, "
          f"smallest radius {min(r1.min(), r2.min()):.3e}, smallest |x|^2 {min((f1 ** 2).sum(1).min(), (f2 ** 2).sum(1).min()):.3e}")
    assert np.abs(r1 - s1[:, [3]]).max() <= tol and np.abs(r2 - s2[:, [3]]).max() <= tol
    if kind == "near":
        for f, rad in ((f1, r1), (f2, r2)):                    # the origin really is nearer to every point than its 3rd neighbour
            assert np.all(rad[:, 0] > (f.astype(np.float64) ** 2).sum(1) + 2 * tol)
    in1, in2 = mc.ref_flags(d12, s1[:, [3]], s2[:, [3]])
    amb1, amb2 = mc.ambiguous_flags(d12, s1[:, [3]], s2[:, [3]], tol)
    u_in, v_in = _flags(f1, f2, s1[:, [3]], s2[:, [3]])
    assert not ((u_in.astype(bool) != in1) & ~amb1).any() and not ((v_in.astype(bool) != in2) & ~amb2).any()
    assert amb1.mean() <= 0.01 and amb2.mean() <= 0.01


def test_n_equals_k1_and_identical_sets():
    r = mc.reference(4)
    f = r["f1"][:4]                                            # N = k1 = 4: the radius is the largest of a row's distances
    radii = ev.ManifoldEstimator().manifold_radii(f)
    assert np.abs(radii[:, 0] - mc.sqdist(f, f).max(1)).max() <= mc.tol_d(f, f)
    with pytest.raises(ValueError, match="max\\(nhood_sizes\\)"):
        ev.ManifoldEstimator().manifold_radii(_dev(f[:3]))
    for index in (1, 4):
        f = mc.reference(index)["f1"]
        assert ev.compute_prec_recall(f, f.copy()) == (1.0, 1.0)


def test_results_do_not_depend_on_chunking_or_run():
    """row_batch_size / col_batch_size cut the work into launches (and the radii into merged partial lists); not one bit changes."""
    for index in (0, 1):
        r = mc.reference(index)
        out = []
        for rb, cb in ((10000, 10000), (64, 64), (100, 64), (64, 100), (100, 100), (10000, 10000)):
            est = ev.ManifoldEstimator(row_batch_size=rb, col_batch_size=cb, nhood_sizes=(3, 5))
            r1, r2 = est.manifold_radii(r["f1"]), est.manifold_radii(r["f2"])
            pr = est.evaluate_pr(r["f1"], r1, r["f2"], r2)
            out.append((r1, r2, *est.last_status, *pr))
        for other in out[1:]:
            for a, b in zip(out[0], other):
                assert a.dtype == b.dtype and np.array_equal(a, b)


def test_non_finite_features_are_refused():
    f = mc.reference(4)["f1"].copy()
    for bad in (np.nan, np.inf, -np.inf):
        g = f.copy()
        g[17, 3] = bad
        with pytest.raises(ValueError, match="NaN or inf"):
            ev.ManifoldEstimator().manifold_radii(g)
        with pytest.raises(ValueError, match="NaN or inf"):
            ev.compute_prec_recall(f, g)
        with pytest.raises(ValueError, match="NaN or inf"):
            ev.compute_statistics(g)


def _check_statistics(x, label):
    """|mu - ref| <= 4 N eps mean|x| and |sigma - ref|_ij <= 4 N eps sqrt(ref_ii ref_jj): the bound on a length-N f64 sum in any
    order (through Cauchy-Schwarz on sum |a b| for the covariance), with the factor 4 covering the centring and the division."""
    n = len(x)
    st = ev.compute_statistics(x)
    mu, sigma = mc.ref_statistics(x)
    assert st.mu.dtype == np.float64 and st.sigma.dtype == np.float64 and st.mu.shape == mu.shape and st.sigma.shape == sigma.shape
    mu_bound = 4 * n * EPS64 * np.abs(x.astype(np.float64)).mean(0)
    sd = np.sqrt(np.diagonal(sigma))
    bound = 4 * n * EPS64 * np.outer(sd, sd)
    err = np.abs(st.sigma - sigma)
    print(f"[statistics {label} {x.shape}] max sigma err / bound = {np.max(err / np.maximum(bound, 1e-300)):.4f}, "
          f"max mu err / bound = {np.max(np.abs(st.mu - mu) / np.maximum(mu_bound, 1e-300)):.4f}")
    assert np.all(np.abs(st.mu - mu) <= mu_bound)
    assert np.all(err <= bound)
    assert np.array_equal(st.sigma, st.sigma.T)
    again = ev.compute_statistics(_dev(x))
    assert np.array_equal(again.mu, st.mu) and np.array_equal(again.sigma, st.sigma)
    return st


@pytest.mark.parametrize("shape", [(257, 23), (300, 40), (130, 2023), (3, 5)])
def test_statistics_against_float64(shape):
    _check_statistics(mc.make_features(shape[0], 2, shape[1], 7)[0], "low-rank")


def test_statistics_survive_cancellation():
    """Features 100 + 0.01 randn: the covariance (1e-4) is 1e-8 of E[x x^T] (1e4).  The centred two-pass form keeps the bound; a
    one-pass E[x x^T] - mu mu^T loses 8 of its 16 digits and misses it by orders of magnitude."""
    rng = np.random.default_rng(2)
    x = (100 + 0.01 * rng.standard_normal((300, 40))).astype(np.float32)
    _check_statistics(x, "cancellation")
    x64 = x.astype(np.float64)
    one_pass = (x64.T @ x64 / 300 - np.outer(x64.mean(0), x64.mean(0))) * 300 / 299
    ref = np.cov(x64, rowvar=False)
    sd = np.sqrt(np.diagonal(ref))
    assert np.abs(one_pass - ref).max() > 100 * (4 * 300 * EPS64 * np.outer(sd, sd)).max()     # the case does tell the two apart


def test_statistics_of_a_single_row():
    x = mc.make_features(1, 3, 5, 0)[0]
    mu = ops.col_mean_f64(_dev(x))
    assert np.array_equal(_np(mu), x[0].astype(np.float64))
    assert np.all(np.isnan(_np(ops.cov_f64(_dev(x), mu))))      # 0 / 0, as np.cov gives for one observation


def test_metrics_from_activations_end_to_end():
    r = mc.reference(0)
    sp1, sp2 = mc.make_features(300, 260, 23, 9)
    m = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2))
    assert sorted(m) == ["fid", "precision", "recall", "sfid"]
    assert all(isinstance(v, float) and np.isfinite(v) for v in m.values())
    ref = {k: ev.FIDStatistics(*mc.ref_statistics(x)) for k, x in (("p1", r["f1"]), ("p2", r["f2"]), ("s1", sp1), ("s2", sp2))}
    print(f"[metrics] {m}; restatement fid {ref['p2'].frechet_distance(ref['p1'])} sfid {ref['s2'].frechet_distance(ref['s1'])}")
    assert m["fid"] == pytest.approx(ref["p2"].frechet_distance(ref["p1"]), rel=1e-8)
    assert m["sfid"] == pytest.approx(ref["s2"].frechet_distance(ref["s1"]), rel=1e-8)
    assert (m["precision"], m["recall"]) == (float(r["precision"][0]), float(r["recall"][0]))
    given = ev.metrics_from_activations((r["f1"], sp1), (_dev(r["f2"]), _dev(sp2)), ref_stats=ev.compute_statistics(r["f1"]),
                                        ref_stats_spatial=ev.compute_statistics(sp1))
    assert given == m
    moved = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2), ref_stats=ref["p2"])      # given statistics are used
    assert moved["fid"] == pytest.approx(0.0, abs=1e-6 * np.trace(ref["p2"].sigma)) and moved["sfid"] == m["sfid"]

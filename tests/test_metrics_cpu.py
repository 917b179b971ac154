"""CPU-only checks of the evaluation metrics: the C ABI exports and refuses what include/vaw_hip.h says, the host surface of
vaw_amd.evaluator keeps the reference's names and refuses bad inputs before anything is uploaded, frechet_distance reproduces the
reference's recorded values, and the inputs of test_gpu_metrics.py are fit for an exact comparison.  No kernel is launched."""
import os
import re
import warnings

import numpy as np
import pytest

import metrics_cases as mc
import abi_cases
import vaw_amd
from vaw_amd import evaluator as ev

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "metrics_fid.npz"))
INT_ENTRIES = ("vaw_row_sqnorms", "vaw_pairwise_ksmallest", "vaw_ksmallest_merge", "vaw_pairwise_within", "vaw_col_mean_f64", "vaw_cov_f64")


def test_symbols_declared_exported_and_built_without_contraction():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    lib = vaw_amd.lib()
    for name in INT_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        abi_cases.assert_bound_as_declared(lib, name)
    assert re.search(r"\bint64_t\s+vaw_pairwise_workspace_bytes\s*\(", hdr)
    assert "vaw_pairwise_workspace_bytes" in vaw_amd.exported_symbols() and hasattr(lib, "vaw_pairwise_workspace_bytes")
    mk = open(os.path.join(REPO, "variance-aware-weight_amd", "csrc", "Makefile")).read()
    assert "metrics.hip" in mk and re.search(r"EXTRA_metrics\s*=\s*-ffp-contract=off", mk)
    for name in ("FIDStatistics", "ManifoldEstimator", "compute_statistics", "compute_prec_recall", "metrics_from_activations"):
        assert getattr(vaw_amd, name) is getattr(ev, name)


def test_workspace_is_linear_in_rows_and_k1_never_n_squared():
    ws = vaw_amd.lib().vaw_pairwise_workspace_bytes
    assert ws(50000, 50000, 4) == 50000 * 4 * 4 * 32          # nu * k1 * 4 bytes * twice the 16 column ranges
    assert ws(50000, 50000, 4) < 50000 * 50000 * 4 // 300
    assert ws(100, 100, 4) == 100 * 4 * 4 * 2 and ws(100, 129, 16) == 100 * 16 * 4 * 4
    assert ws(50000, 10 ** 7, 4) == ws(50000, 50000, 4)       # the number of column ranges is capped
    assert ws(0, 5, 4) == 0 and ws(5, 5, 17) == 0 and ws(5, 5, 0) == 0


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    P = 4096                                                  # a non-null placeholder address, never dereferenced

    def ks(U=P, nu=5, V=P, nv=7, D=3, k1=4, out=P, ws=P, ws_bytes=1 << 20):
        return lib.vaw_pairwise_ksmallest(U, nu, V, nv, D, P, P, k1, out, ws, ws_bytes, None)

    for bad in (dict(k1=0), dict(k1=17), dict(k1=8), dict(nu=0), dict(nv=0), dict(D=0), dict(U=None), dict(V=None), dict(out=None),
                dict(ws=None), dict(ws_bytes=5 * 4 * 4 * 2 - 1), dict(nu=1 << 31)):
        assert ks(**bad) == -1, bad
        assert b"pairwise_ksmallest" in lib.vaw_last_error_string()

    def within(nu=5, nv=7, D=3, Ku=1, Kv=2, u_in=P, v_in=P, ru=P):
        return lib.vaw_pairwise_within(P, nu, P, nv, D, P, P, ru, Ku, P, Kv, u_in, v_in, None)

    for bad in (dict(Ku=0), dict(Ku=5), dict(Kv=0), dict(Kv=5), dict(nu=0), dict(nv=-1), dict(D=0), dict(u_in=None), dict(v_in=None), dict(ru=None)):
        assert within(**bad) == -1, bad
        assert b"pairwise_within" in lib.vaw_last_error_string()
    assert lib.vaw_row_sqnorms(P, 0, 3, P, None) == -1 and lib.vaw_row_sqnorms(None, 2, 3, P, None) == -1
    assert lib.vaw_col_mean_f64(P, 2, 0, P, None) == -1 and lib.vaw_col_mean_f64(P, 2, 3, None, None) == -1
    assert lib.vaw_cov_f64(P, 0, 3, P, P, None) == -1 and lib.vaw_cov_f64(P, 2, 3, P, None, None) == -1
    assert lib.vaw_ksmallest_merge(P, 3, 0, 4, 4, 8, P, None) == -1 and lib.vaw_ksmallest_merge(P, 3, 2, 17, 17, 34, P, None) == -1


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from vaw_amd import ops
    x = torch.zeros(5, 3)
    for call in (lambda: ops.row_sqnorms(x), lambda: ops.col_mean_f64(x), lambda: ops.pairwise_ksmallest(x, x, 2),
                 lambda: ops.cov_f64(x, torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(vaw_amd.VawError):                 # no CPU fallback
            call()


@pytest.mark.parametrize("kind", ["well", "singular"])
def test_frechet_distance_matches_the_reference(kind):
    a = ev.FIDStatistics(GOLD[f"{kind}_mu_a"], GOLD[f"{kind}_sigma_a"])
    b = ev.FIDStatistics(GOLD[f"{kind}_mu_b"], GOLD[f"{kind}_sigma_b"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fd, fd_rev = a.frechet_distance(b), b.frechet_distance(a)
    eps_branch = any("singular product" in str(w.message) for w in caught)
    assert eps_branch == bool(GOLD[f"{kind}_eps_branch"])     # the same branch, hence the same warning or none
    assert fd == pytest.approx(float(GOLD[f"{kind}_fd"]), rel=1e-9) and fd_rev == pytest.approx(float(GOLD[f"{kind}_fd_rev"]), rel=1e-9)
    assert a.frechet_distance(a) == pytest.approx(0.0, abs=1e-6 * float(np.trace(a.sigma)))


def test_frechet_distance_eps_fallback_and_imaginary_check(monkeypatch):
    """The two branches the recorded pairs do not reach, driven through the square root: a non-finite first root warns and is retried
    with eps on both diagonals; a root whose diagonal is not real is refused."""
    s = ev.FIDStatistics(np.zeros(2), np.eye(2))
    seen = []

    def fake(m):
        seen.append(np.array(m))
        return np.full((2, 2), np.nan) if len(seen) == 1 else np.eye(2) * (1 + 1e-3)

    monkeypatch.setattr(ev, "_sqrtm", fake)
    with pytest.warns(UserWarning, match="singular product; adding 0.001 to diagonal"):
        fd = s.frechet_distance(ev.FIDStatistics(np.ones(2), np.eye(2)), eps=1e-3)
    np.testing.assert_allclose(seen[1], np.eye(2) * (1 + 1e-3) ** 2)
    assert fd == pytest.approx(2 + 2 + 2 - 2 * 2 * (1 + 1e-3))
    monkeypatch.setattr(ev, "_sqrtm", lambda m: np.eye(2) * (1 + 0.5j))
    with pytest.raises(ValueError, match="Imaginary component"):
        s.frechet_distance(s)


def test_host_surface_refuses_bad_inputs_with_value_error():
    f = np.zeros((6, 4), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        ev.compute_statistics(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="2-D"):
        ev.ManifoldEstimator().manifold_radii(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="widths differ"):
        ev.compute_prec_recall(f, np.zeros((6, 5), np.float32))
    with pytest.raises(ValueError, match="widths differ"):
        ev.ManifoldEstimator().evaluate_pr(f, np.zeros((6, 1)), np.zeros((6, 5), np.float32), np.zeros((6, 1)))
    with pytest.raises(ValueError, match="widths differ"):
        ev.metrics_from_activations((f, f), (f, np.zeros((6, 3), np.float32)))
    with pytest.raises(ValueError, match="max\\(nhood_sizes\\)"):
        ev.ManifoldEstimator().manifold_radii(np.zeros((3, 4), np.float32))           # N = 3 <= k = 3
    with pytest.raises(ValueError, match="max\\(nhood_sizes\\)"):
        ev.compute_prec_recall(f, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="radii_1"):
        ev.ManifoldEstimator().evaluate_pr(f, np.zeros((5, 1)), f, np.zeros((6, 1)))
    with pytest.raises(ValueError, match="nhood_sizes"):
        ev.ManifoldEstimator(nhood_sizes=(16,))
    with pytest.raises(ValueError, match="pair"):
        ev.metrics_from_activations(f, (f, f))
    with pytest.raises(NotImplementedError):
        ev.ManifoldEstimator().evaluate(f, f, f)
    with pytest.raises(TypeError):
        ev.ManifoldEstimator(session=None)                                             # the reference's session argument is gone


@pytest.mark.parametrize("index", range(len(mc.CASES)), ids=mc.CASE_IDS)
def test_inputs_are_fit_for_the_gpu_test(index):
    """On the float64 restatement alone: precision and recall are away from 0 and 1, no two of a row's first k + 2 sorted distances
    are closer than the band 2 tolD (two values that each move by tolD keep their order), and no flag is ambiguous, so the GPU test
    may demand every flag and precision / recall exactly.  float32 numpy, an independent f32 path, flips no flag either."""
    r = mc.reference(index)
    for v in (*r["precision"], *r["recall"]):
        assert 0.05 <= v <= 0.98
    k = max(r["nhood"])
    gap = min(mc.min_gap(r["sorted1"], k + 2), mc.min_gap(r["sorted2"], k + 2))
    assert gap >= 2 * r["tol"], (gap, r["tol"])
    assert int(r["amb1"].sum()) == 0 and int(r["amb2"].sum()) == 0
    f1, f2 = r["f1"], r["f2"]
    n1, n2 = (f1 * f1).sum(1, dtype=np.float32), (f2 * f2).sum(1, dtype=np.float32)
    d32 = np.maximum(n1[:, None] - 2 * (f1 @ f2.T) + n2[None, :], 0)
    err = float(np.abs(d32 - r["d12"]).max())
    print(f"[metrics inputs {mc.CASE_IDS[index]}] float32 numpy vs float64: max |d32 - d64| = {err:.3e} = {err / r['tol']:.3f} tolD")
    assert d32.dtype == np.float32 and err <= r["tol"]       # the bound asked of the kernel holds for this f32 evaluation too
    in1, in2 = mc.ref_flags(d32, r["radii1"].astype(np.float32), r["radii2"].astype(np.float32))
    assert np.array_equal(in1, r["in1"]) and np.array_equal(in2, r["in2"])

"""CPU-only checks of KID and density / coverage: the C ABI exports and refuses what include/vaw_hip.h says, the host surface of
vaw_amd.evaluator refuses bad inputs before anything is uploaded, the subset index stream is the recorded one, and the inputs of
test_gpu_kid_dc.py are fit for the comparison it makes.  No kernel is launched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import kid_dc_cases as kc
import metrics_cases as mc
import abi_cases
import vaw_amd
from vaw_amd import evaluator as ev, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(REPO, "tests", "golden", "kid_dc.json")))
INT_ENTRIES = ("vaw_pairwise_polysum", "vaw_pairwise_count_within")
SIZE_ENTRIES = ("vaw_pairwise_polysum_workspace_bytes", "vaw_pairwise_count_workspace_bytes")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    lib = vaw_amd.lib()
    for name in INT_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        abi_cases.assert_bound_as_declared(lib, name)
    for name in SIZE_ENTRIES:
        assert re.search(r"\bint64_t\s+" + name + r"\s*\(", hdr), name
        assert name in vaw_amd.exported_symbols() and getattr(lib, name).restype is ctypes.c_int64
        abi_cases.assert_bound_as_declared(lib, name)
    # the declared parameter lists and the bound ones agree in length and in where the doubles are
    for name in INT_ENTRIES:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")
        protos = getattr(lib, name).argtypes
        assert len(params) == len(protos), name
        assert [p.split()[0] == "double" and "*" not in p for p in params] == [t is ctypes.c_double for t in protos], name
    for name in ("polynomial_mmd2", "kid_subset_scores", "kid_subset_indices", "compute_kid", "compute_density_coverage"):
        assert getattr(vaw_amd, name) is getattr(ev, name)
    for name in ("compute_kid", "compute_density_coverage"):
        assert callable(getattr(ev.Evaluator, name))
    assert callable(ev.ManifoldEstimator.evaluate_dc)


def test_workspaces_are_linear_in_rows_never_n_squared():
    poly, count = vaw_amd.lib().vaw_pairwise_polysum_workspace_bytes, vaw_amd.lib().vaw_pairwise_count_workspace_bytes
    assert poly(1000, 1000, 100) == 100 * 1000 * 8 * 16               # batches * nu * 8 bytes * twice the 8 column ranges
    assert poly(50000, 50000, 1) == 50000 * 8 * 32 and poly(50000, 10 ** 7, 1) == poly(50000, 50000, 1)
    assert poly(100, 100, 3) == 3 * 100 * 8 * 2 and poly(100, 129, 1) == 100 * 8 * 4
    assert poly(0, 5, 1) == 0 and poly(5, 0, 1) == 0 and poly(5, 5, 0) == 0
    assert count(50000, 50000, 1) == 50000 * 4 * 32 and count(50000, 50000, 4) == 4 * count(50000, 50000, 1)
    assert count(100, 129, 2) == 100 * 2 * 4 * 4
    assert count(0, 5, 1) == 0 and count(5, 5, 0) == 0 and count(5, 5, 5) == 0


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    P = 4096                                                  # a non-null placeholder address, never dereferenced
    inf, nan = float("inf"), float("nan")

    def poly(U=P, nu=5, V=P, nv=7, D=3, batches=2, gamma=0.5, coef0=1.0, degree=3, out=P, ws=P, ws_bytes=1 << 20):
        return lib.vaw_pairwise_polysum(U, nu, V, nv, D, None, None, batches, gamma, coef0, degree, 1, out, ws, ws_bytes, None)

    for bad in (dict(U=None), dict(V=None), dict(out=None), dict(ws=None), dict(nu=0), dict(nv=0), dict(D=0), dict(batches=0), dict(nu=-3),
                dict(degree=0), dict(degree=9), dict(degree=-1), dict(ws_bytes=2 * 5 * 2 * 8 - 1), dict(nu=1 << 31), dict(nv=1 << 31),
                dict(gamma=inf), dict(gamma=nan), dict(coef0=-inf), dict(coef0=nan), dict(batches=1 << 30, nu=1 << 20)):
        assert poly(**bad) == -1, bad
        assert b"vaw_pairwise_polysum" in lib.vaw_last_error_string(), bad

    def count(U=P, nu=5, V=P, nv=7, D=3, nrm=P, rv=P, Kv=2, u_count=P, v_in=P, ws=P, ws_bytes=1 << 20):
        return lib.vaw_pairwise_count_within(U, nu, V, nv, D, nrm, P, rv, Kv, u_count, v_in, ws, ws_bytes, None)

    for bad in (dict(U=None), dict(V=None), dict(nrm=None), dict(rv=None), dict(u_count=None), dict(v_in=None), dict(ws=None), dict(nu=0),
                dict(nv=-1), dict(D=0), dict(Kv=0), dict(Kv=5), dict(ws_bytes=5 * 2 * 2 * 4 - 1), dict(nu=1 << 31), dict(nv=1 << 31)):
        assert count(**bad) == -1, bad
        assert b"vaw_pairwise_count_within" in lib.vaw_last_error_string(), bad


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    x = torch.zeros(5, 3)
    i32, u8 = torch.zeros(5, 1, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.uint8)
    for call in (lambda: ops.pairwise_polysum(x, x, 0.5, 1.0, 3),
                 lambda: ops.pairwise_count_within(x, x, torch.zeros(5), torch.zeros(5), torch.zeros(5, 1), i32, u8)):
        with pytest.raises(vaw_amd.VawError):                 # no CPU fallback
            call()


def test_host_surface_refuses_bad_inputs_with_value_error():
    f, g = np.zeros((8, 4), np.float32), np.zeros((6, 4), np.float32)
    wide = np.zeros((8, 5), np.float32)
    for fn in (ev.kid_subset_scores, ev.compute_kid, ev.Evaluator().compute_kid):
        for kw in (dict(subset_size=1), dict(subset_size=7), dict(subset_size=9), dict(num_subsets=0), dict(degree=0), dict(degree=9),
                   dict(degree=2.5), dict(gamma=float("inf")), dict(coef0=float("nan"))):
            with pytest.raises(ValueError, match="subset_size|num_subsets|degree|finite"):
                fn(f, g, **{**dict(num_subsets=2, subset_size=4), **kw})
        with pytest.raises(ValueError, match="widths differ"):
            fn(f, wide, num_subsets=2, subset_size=4)
    with pytest.raises(ValueError, match="widths differ"):
        ev.polynomial_mmd2(f, wide)
    with pytest.raises(ValueError, match="degree"):
        ev.polynomial_mmd2(f, g, degree=9)
    with pytest.raises(ValueError, match="at least 2"):
        ev.polynomial_mmd2(f, g[:1])
    with pytest.raises(ValueError, match="2-D"):
        ev.polynomial_mmd2(np.zeros(5, np.float32), g)
    for fn in (ev.compute_density_coverage, ev.Evaluator().compute_density_coverage):
        with pytest.raises(ValueError, match="widths differ"):
            fn(f, wide)
        with pytest.raises(ValueError, match="nearest_k"):
            fn(g[:5], f)                                      # N = 5 <= nearest_k = 5
        with pytest.raises(ValueError, match="nearest_k"):
            fn(f, g, nearest_k=0)
        with pytest.raises(ValueError, match="nearest_k"):
            fn(f, g, nearest_k=16)
    est = ev.ManifoldEstimator()
    with pytest.raises(ValueError, match="widths differ"):
        est.evaluate_dc(f, np.zeros((8, 1)), wide)
    with pytest.raises(ValueError, match="radii_real"):
        est.evaluate_dc(f, np.zeros((7, 1)), g)
    with pytest.raises(ValueError, match="radii_real"):
        est.evaluate_dc(f, np.zeros((8, 2)), g)
    with pytest.raises(ValueError, match="radii_real"):
        est.evaluate_dc(f, np.zeros(8), g)
    with pytest.raises(ValueError, match="holds 0"):
        ev.ManifoldEstimator(nhood_sizes=(0,)).evaluate_dc(f, np.zeros((8, 1)), g)
    with pytest.raises(NotImplementedError):
        est.evaluate(f, f, f)                                 # realism scores stay unbuilt


def test_metrics_from_activations_checks_its_new_options_before_any_upload():
    f, g = np.zeros((8, 4), np.float32), np.zeros((6, 4), np.float32)
    for kw in (dict(kid=dict(subset_size=7)), dict(kid=dict(subset_size=4, num_subsets=0)), dict(kid=dict(subset_size=4, degree=9)),
               dict(kid=True),                                 # the default subset_size = 1000 is larger than either set
               dict(kid=3), dict(kid=dict(subset_size=4, subsets=3)), dict(density_coverage=8), dict(density_coverage=0),
               dict(density_coverage=2.5)):
        with pytest.raises(ValueError, match="metrics_from_activations"):
            ev.metrics_from_activations((f, f), (g, g), **kw)
    with pytest.raises(ValueError, match="widths differ"):    # the earlier checks still come first
        ev.metrics_from_activations((f, f), (g, np.zeros((6, 3), np.float32)), kid=dict(subset_size=4), density_coverage=True)
    with pytest.raises(ValueError, match="pair"):
        ev.metrics_from_activations(f, (g, g), kid=True)


def test_subset_index_stream_is_the_recorded_protocol():
    for rec in GOLD["subset_draws"]:
        args = (rec["n_ref"], rec["n_sample"], rec["num_subsets"], rec["subset_size"], rec["seed"])
        ri, si = ev.kid_subset_indices(*args)
        assert ri.dtype == np.int32 and si.dtype == np.int32 and ri.shape == si.shape == (rec["num_subsets"], rec["subset_size"])
        assert ri.tolist() == rec["ref_idx"] and si.tolist() == rec["sample_idx"]
        want = kc.subset_indices(*args)
        assert np.array_equal(ri, want[0]) and np.array_equal(si, want[1])
        assert all(len(set(row)) == len(row) for row in ri.tolist() + si.tolist())           # without replacement
    ri, si = ev.kid_subset_indices(300, 260, 100, 129, 5)
    want = kc.subset_indices(300, 260, 100, 129, 5)
    assert np.array_equal(ri, want[0]) and np.array_equal(si, want[1]) and ri.max() < 300 and si.max() < 260


@pytest.mark.parametrize("index", range(len(mc.CASES)), ids=kc.CASE_IDS)
def test_float_inputs_are_fit_for_the_gpu_test(index):
    """On the float64 restatement alone.  Few generated rows have a pair within 2 tolD of its radius (the GPU test brackets those rows'
    counts), no coverage flag is ambiguous (it demands every flag), and the wrong estimators are further from the right one than 100
    times the tolerance it grants."""
    r = kc.reference(index)
    share = float(r["ambiguous_rows"].mean())
    print(f"[kid/dc inputs {kc.CASE_IDS[index]}] density {r['density'][0]:.4f} coverage {r['coverage'][0]:.4f} mmd2 {r['mmd2']:.4f} "
          f"+- {r['mmd2_bound']:.2e}; pairs within 2 tolD of a radius {r['near_pairs']}, share of rows {share:.4f}")
    assert share <= 0.02 and int(r["ambiguous_flags"].sum()) == 0
    assert 0.05 <= r["coverage"][0] <= 0.98 and r["density"][0] > 0.05
    assert np.all(r["counts_lo"] <= r["counts"]) and np.all(r["counts"] <= r["counts_hi"])
    f1, f2, gamma = r["f1"], r["f2"], r["gamma"]
    for variant in ("diagonal", "biased"):
        wrong = kc.mmd2(f1, f2, gamma, kc.COEF0, kc.DEGREE, variant)
        assert abs(wrong - r["mmd2"]) > 100 * r["mmd2_bound"], variant
    for key in ("11", "22"):                                  # a row sum with its diagonal term is not one without
        assert np.all(r["rows_" + key] - r["rows_" + key + "_skip"] > 100 * r["bound_" + key + "_skip"])
    assert np.all(r["bound_12"] < 1e-4 * np.abs(r["rows_12"]))                              # the tolerance is a tight one


@pytest.mark.parametrize("index", range(len(kc.EXACT_CASES)), ids=kc.EXACT_IDS)
def test_exact_inputs_hold_ties_and_copies(index):
    """Integer features: d == r ties and d == 0 copies occur, every value is exact in f32 (distances) and f64 (kernel sums), and
    `<=` in place of `<` changes counts, density and coverage flags."""
    r = kc.exact_reference(index)
    assert r["ties"] >= 20 and r["zeros"] >= 30
    assert np.array_equal(r["d"], r["d"].astype(np.float32)) and np.array_equal(r["radii"], r["radii"].astype(np.float32))
    assert int((r["counts_le"] - r["counts"]).sum()) >= 20 and kc.density_coverage(r["counts_le"], r["flags_le"], (5,))[0][0] > r["density"][0]
    real, fake = r["real"].astype(np.float64), r["fake"].astype(np.float64)
    k = (16 + real @ fake.T) ** 3                              # integers: (gamma dot + coef0)^3 = (16 + dot)^3 / 2^12
    assert k.max() < 2 ** 40 and np.array_equal(r["rows_12"] * 4096, k.sum(1))
    for variant in ("diagonal", "biased"):
        assert kc.mmd2(real, fake, kc.EXACT_GAMMA, kc.COEF0, kc.DEGREE, variant) != r["mmd2"]

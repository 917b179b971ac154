"""CPU-only checks of the Inception score: the float64 restatement of inception_cases.py reproduces the values recorded from the
reference (tests/golden/INCEPTION_SCORE.md), the inputs of test_gpu_inception.py are fit for their bounds, and the host surface of
vaw_amd.evaluator keeps the reference's names and refuses bad inputs before anything is uploaded.  No kernel is launched."""
import os
import re

import numpy as np
import pytest

import inception_cases as ic
import abi_cases
import vaw_amd
from vaw_amd import evaluator as ev

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_ENTRIES = ("vaw_head_logits", "vaw_is_rows", "vaw_is_colsums", "vaw_is_finish")
GOLD, GOLD_GAP = ic.golden()
FINITE = [k for k in GOLD if k != "zero"]


@pytest.mark.parametrize("name", list(GOLD))
def test_restatement_matches_the_fixture(name):
    g = GOLD[name]
    got = ic.score(g["preds"], g["split"])
    print(f"[fixture {name}] restatement {got!r} recorded score_f64 {g['score_f64']!r}")
    assert abs(got - g["score_f64"]) <= 1e-13 * g["score_f64"]


@pytest.mark.parametrize("name", FINITE)
def test_reference_agrees_with_float64_within_its_f32_arithmetic(name):
    """The reference sums rows * C float32 terms p g (numpy sums pairwise): its kl is off by at most
    2^-24 (log2(rows C) + 8) mean_i sum_c |p g|, which is the relative gap of exp(kl); 8 covers log, the subtraction, the product,
    the mean and exp.  The largest split stands for all (the score is the mean of the splits' scores)."""
    g = GOLD[name]
    rows = min(g["split"], len(g["preds"]))
    bound = 2.0 ** -24 * (np.log2(rows * g["preds"].shape[1]) + 8) * ic.mean_abs_terms(g["preds"], g["split"])
    gap = abs(g["score_ref"] - g["score_f64"]) / g["score_f64"]
    print(f"[fixture {name}] |score_ref - score_f64| / score_f64 = {gap:.3e}, bound {bound:.3e}, recorded largest gap {GOLD_GAP:.3e}")
    assert gap <= bound and gap <= GOLD_GAP


def test_zero_probabilities_reference_nan_restatement_finite():
    g = GOLD["zero"]
    assert int((g["preds"] == 0).sum()) > 0
    assert np.isnan(g["score_ref"]) and np.isfinite(g["score_f64"]) and np.isfinite(ic.score(g["preds"], g["split"]))
    p = g["preds"][:g["split"]]
    with np.errstate(divide="ignore", invalid="ignore"):          # the reference's own expression on the first split
        assert np.isnan(np.mean(np.sum(p * (np.log(p) - np.log(np.expand_dims(np.mean(p, 0), 0))), 1)))


@pytest.mark.parametrize("index", range(len(ic.CASES)), ids=ic.CASE_IDS)
def test_inputs_are_fit_for_the_gpu_test(index):
    """On the restatement alone: the scored cases lie between 1.2 and C / 2 (a constant answer fails), no float32 probability is 0
    (so the zero limit plays no part in them), and float32 numpy -- an independent f32 evaluation -- meets the logit tolerance."""
    r = ic.reference(index)
    n, d, c, split, _ = ic.CASES[index]
    l32 = r["x"] @ r["w"]
    err = np.abs(l32.astype(np.float64) - r["logits"])
    e32 = np.exp(l32 - l32.max(1, keepdims=True))
    p32 = e32 / e32.sum(1, keepdims=True)
    s32 = ic.score(p32, split)
    print(f"[inception inputs {ic.CASE_IDS[index]}] score {r['score']:.6f}, splits {r['split_scores'].min():.4f} .. {r['split_scores'].max():.4f}, "
          f"float32 numpy: score rel {abs(s32 - r['score']) / r['score']:.2e}, logits max err / tol {np.max(err / r['tol']):.3f}, "
          f"smallest p {p32.min():.2e}; delta {r['delta']:.3e}, score tol {r['score_tol']:.3e}")
    assert l32.dtype == np.float32 and p32.dtype == np.float32 and np.all(err <= r["tol"])
    assert p32.min() > 0
    if index in ic.SCORED:
        assert 1.2 <= r["score"] <= c / 2
    else:
        assert np.all(np.abs(r["split_scores"] - 1) <= 1e-12)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    lib = vaw_amd.lib()
    for name in INT_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
        abi_cases.assert_bound_as_declared(lib, name)
    for name in ("Evaluator", "compute_inception_score", "inception_score_from_probs", "inception_split_scores"):
        assert getattr(vaw_amd, name) is getattr(ev, name)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    P = 4096                                                  # a non-null placeholder address, never dereferenced

    def head(X=P, n=5, D=3, Wt=P, C=7, out=P, ld=7):
        return lib.vaw_head_logits(X, n, D, Wt, C, out, ld, None)

    for bad in (dict(n=0), dict(D=0), dict(C=0), dict(ld=6), dict(X=None), dict(Wt=None), dict(out=None), dict(n=1 << 31)):
        assert head(**bad) == -1, bad
        assert b"vaw_head_logits" in lib.vaw_last_error_string()
    assert lib.vaw_is_rows(P, 0, 3, 3, 0, P, P, None) == -1 and lib.vaw_is_rows(P, 2, 3, 2, 0, P, P, None) == -1
    assert lib.vaw_is_rows(None, 2, 3, 3, 0, P, P, None) == -1 and lib.vaw_is_rows(P, 2, 3, 3, 1, P, None, None) == -1
    assert lib.vaw_is_colsums(P, P, 2, 3, 3, 0, 0, 0, P, None) == -1 and lib.vaw_is_colsums(P, P, 2, 3, 3, 0, -1, 5, P, None) == -1
    assert lib.vaw_is_colsums(P, None, 2, 3, 3, 0, 0, 5, P, None) == -1 and lib.vaw_is_colsums(P, P, 2, 3, 3, 0, 0, 5, None, None) == -1
    assert lib.vaw_is_finish(P, P, 0, 3, 5, P, None) == -1 and lib.vaw_is_finish(P, P, 4, 3, 0, P, None) == -1
    assert lib.vaw_is_finish(P, None, 4, 3, 5, P, None) == -1


def test_wrappers_refuse_cpu_tensors():
    import torch
    from vaw_amd import ops
    x, wt = torch.zeros(5, 3), torch.zeros(4, 3)
    d = torch.zeros(5, dtype=torch.float64)
    for call in (lambda: ops.head_logits(x, wt), lambda: ops.is_rows(x), lambda: ops.is_colsums(x, d, 0, 5, torch.zeros(1, 3, dtype=torch.float64)),
                 lambda: ops.is_finish(d, torch.zeros(1, 3, dtype=torch.float64), 5)):
        with pytest.raises(vaw_amd.VawError):                 # no CPU fallback
            call()


def test_host_surface_refuses_bad_inputs(tmp_path):
    x = np.ones((6, 4), np.float32)
    w = np.ones((4, 3), np.float32)
    with pytest.raises(ValueError, match="no softmax_weight"):
        ev.Evaluator().compute_inception_score(x)
    with pytest.raises(ValueError, match="wide"):
        ev.compute_inception_score(x, np.ones((5, 3), np.float32))
    with pytest.raises(ValueError, match="wide"):
        ev.Evaluator(softmax_weight=np.ones((5, 3), np.float32)).compute_inception_score(x)
    with pytest.raises(ValueError, match="2-D \\[D, C\\]"):
        ev.compute_inception_score(x, np.ones(4, np.float32))
    with pytest.raises(ValueError, match="split_size"):
        ev.compute_inception_score(x, w, split_size=0)
    with pytest.raises(ValueError, match="split_size"):
        ev.inception_score_from_probs(np.full((6, 3), 1 / 3, np.float32), split_size=0)
    with pytest.raises(ValueError, match="softmax_batch_size"):
        ev.compute_inception_score(x, w, softmax_batch_size=0)
    with pytest.raises(ValueError, match="non-negative"):
        ev.inception_score_from_probs(np.array([[0.5, 0.6], [1.2, -0.2]], np.float32))
    with pytest.raises(ValueError, match="non-negative"):
        ev.inception_score_from_probs(np.array([[0.5, np.nan]], np.float32))
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[1, 2] = bad
        with pytest.raises(ValueError, match="NaN or inf"):
            ev.compute_inception_score(x, wb)
    with pytest.raises(ValueError, match="empty"):
        ev.compute_inception_score(np.zeros((0, 4), np.float32), w)
    with pytest.raises(ValueError, match="2-D"):
        ev.compute_inception_score(np.zeros(4, np.float32), w)
    with pytest.raises(ValueError, match="wide"):
        ev.metrics_from_activations((x, x), (x, x), softmax_weight=np.ones((5, 3), np.float32))
    np.savez(tmp_path / "other.npz", logits=w)
    with pytest.raises(ValueError, match="no array named softmax_weight"):
        ev.Evaluator(softmax_weight=str(tmp_path / "other.npz"))
    np.savez(tmp_path / "head.npz", softmax_weight=w)
    np.save(tmp_path / "head.npy", w)
    for path in (tmp_path / "head.npz", str(tmp_path / "head.npy")):
        e = ev.Evaluator(softmax_weight=path)
        assert (e.softmax_head.width, e.softmax_head.classes) == (4, 3)
    with pytest.raises(NotImplementedError, match="feature extractor"):
        ev.Evaluator().compute_activations([np.zeros((1, 8, 8, 3))])
    with pytest.raises(NotImplementedError, match="feature extractor"):
        ev.Evaluator().read_activations("batch.npz")
    with pytest.raises(TypeError):
        ev.Evaluator(session=None)                            # the reference's session argument is gone
    assert isinstance(ev.Evaluator().manifold_estimator, ev.ManifoldEstimator)


def test_read_statistics_uses_the_file_when_it_has_them(tmp_path):
    mu, sigma = np.arange(3.0), np.eye(3)
    np.savez(tmp_path / "ref.npz", arr_0=np.zeros((2, 2)), mu=mu, sigma=sigma, mu_s=mu + 1, sigma_s=2 * sigma)
    a, b = ev.Evaluator().read_statistics(str(tmp_path / "ref.npz"), None)
    assert isinstance(a, ev.FIDStatistics) and np.array_equal(a.mu, mu) and np.array_equal(a.sigma, sigma)
    assert np.array_equal(b.mu, mu + 1) and np.array_equal(b.sigma, 2 * sigma)

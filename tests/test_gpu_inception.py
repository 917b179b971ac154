"""The Inception-score kernels (csrc/metrics.hip) and vaw_amd.evaluator's compute_inception_score on the GPU against the float64
restatement of inception_cases.py and the values recorded from the reference.  Run on the MI355X box:
pytest -m gpu tests/test_gpu_inception.py.

Logit tolerance.  Per element 3.5e-7 * sum_k |x_ik w_kc|: the bound test_gpu_metrics.py derives for an f32 MFMA chain up to
K = 4096.  Reduction tolerance.  Given f32 logits, the device's float64 softmax and sums against float64 numpy: four sums of at most
max(C, rows) <= 5000 terms at 1.1e-16 per term are 2.2e-12 in ln score; 1e-11 leaves about 4x for exp / log.  End to end the logit
error delta propagates to ln score as 4 delta + 2 delta mean_i sum_c p |g| (inception_cases.score_tol).  The bounds come from the
number formats, not from what the kernels were seen to give; every test prints its measured figure before it asserts."""
import numpy as np
import pytest
import torch

import inception_cases as ic
import metrics_cases as mc

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import evaluator as ev, ops

DEV = "cuda"
REDUCTION_TOL = 1e-11
CASE_IDX = range(len(ic.CASES))
GOLD, GOLD_GAP = ic.golden()


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)      # a copy: the shared references are read-only arrays


def _np(t):
    return t.cpu().numpy()


def _wt(w):
    return _dev(np.ascontiguousarray(w.T))


@pytest.mark.parametrize("index", CASE_IDX, ids=ic.CASE_IDS)
def test_logits_against_float64(index):
    r = ic.reference(index)
    x, wt = _dev(r["x"]), _wt(r["w"])
    got = _np(ops.head_logits(x, wt))
    err = np.abs(got.astype(np.float64) - r["logits"])
    print(f"[logits {ic.CASE_IDS[index]}] max |got - ref| / tol = {np.max(err / r['tol']):.4f}, max |got - ref| = {err.max():.3e}")
    assert got.dtype == np.float32 and got.shape == r["logits"].shape
    assert np.all(err <= r["tol"])
    assert np.array_equal(got, _np(ops.head_logits(x, wt)))


@pytest.mark.parametrize("index", CASE_IDX, ids=ic.CASE_IDS)
def test_reduction_against_float64_on_the_device_logits(index):
    r = ic.reference(index)
    logits = _np(ops.head_logits(_dev(r["x"]), _wt(r["w"])))
    ref = ic.split_scores(ic.softmax64(logits), r["split"])
    got = ev.inception_split_scores(r["x"], r["w"], r["split"])
    gap = np.abs(np.log(got) - np.log(ref))
    print(f"[reduction {ic.CASE_IDS[index]}] {len(ref)} splits, max |ln dev - ln f64| = {gap.max():.3e} (bound {REDUCTION_TOL:.0e})")
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.all(gap <= REDUCTION_TOL)


@pytest.mark.parametrize("name", list(GOLD))
def test_from_probs_on_the_fixture(name):
    """The reference's second half on its own recorded float32 preds; in the zero case the reference gave NaN and the device must
    give the finite float64 value."""
    g = GOLD[name]
    got = ev.inception_split_scores_from_probs(g["preds"], g["split"])
    ref = ic.split_scores(g["preds"], g["split"])
    score = ev.inception_score_from_probs(g["preds"], g["split"])
    gap = max(np.abs(np.log(got) - np.log(ref)).max(), abs(np.log(score) - np.log(g["score_f64"])))
    print(f"[from probs {name}] score {score!r}, recorded score_f64 {g['score_f64']!r}, max |ln dev - ln f64| = {gap:.3e}")
    assert isinstance(score, float) and np.isfinite(score) and score == float(np.mean(got))
    assert gap <= REDUCTION_TOL
    assert score == ev.inception_score_from_probs(_dev(g["preds"]), g["split"])


@pytest.mark.parametrize("index", CASE_IDX, ids=ic.CASE_IDS)
def test_compute_inception_score_against_float64(index):
    r = ic.reference(index)
    got = ev.compute_inception_score(r["x"], r["w"], r["split"])
    gap = abs(np.log(got) - np.log(r["score"]))
    print(f"[score {ic.CASE_IDS[index]}] got {got!r} ref {r['score']!r}, |d ln score| = {gap:.3e}, bound {r['score_tol']:.3e}")
    assert isinstance(got, float)
    assert gap <= r["score_tol"]
    if index not in ic.SCORED:
        assert abs(got - 1.0) <= 1e-12
        assert np.all(np.abs(ev.inception_split_scores(r["x"], r["w"], r["split"]) - 1.0) <= 1e-12)


@pytest.mark.parametrize("name", [k for k in GOLD if k != "zero"])
def test_compute_inception_score_against_the_reference(name):
    """score_ref is the reference's float32 result; it lies within the recorded f32 gap of the float64 value of its preds, which the
    device meets to the propagated logit tolerance."""
    g = GOLD[name]
    delta = float(ic.logit_tol(g["acts"], g["w"]).max())
    bound = ic.score_tol(delta, g["preds"], g["split"]) - np.log1p(-GOLD_GAP)
    got = ev.Evaluator(softmax_weight=g["w"], softmax_batch_size=g["batch"]).compute_inception_score(g["acts"], g["split"])
    gap = abs(np.log(got) - np.log(g["score_ref"]))
    print(f"[reference {name}] got {got!r} score_ref {g['score_ref']!r}, |d ln score| = {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


@pytest.mark.parametrize("index", [0, 2], ids=[ic.CASE_IDS[0], ic.CASE_IDS[2]])
def test_score_does_not_depend_on_batching_placement_or_run(index):
    r = ic.reference(index)
    first = ev.inception_split_scores(r["x"], r["w"], r["split"])
    for batch in (None, 1, 100, 128):
        again = ev.inception_split_scores(r["x"], r["w"], r["split"], softmax_batch_size=batch)
        assert np.array_equal(first, again), batch
    assert np.array_equal(first, ev.inception_split_scores(_dev(r["x"]), _dev(r["w"]), r["split"], softmax_batch_size=100))
    assert np.array_equal(first, ev.inception_split_scores(torch.from_numpy(r["x"].astype(np.float64)), r["w"].astype(np.float64), r["split"]))
    assert ev.compute_inception_score(r["x"], r["w"], r["split"], softmax_batch_size=1) == float(np.mean(first))


def test_a_huge_row_changes_only_its_own_split():
    """129 rows in splits of 128: row 128 is alone in a second row tile and a second split.  Scaled by 1e3 its logits are thousands
    apart (probabilities underflow even in float64: the zero limit), and split 0 keeps every bit."""
    r = ic.reference(2)
    x = r["x"][:129].copy()
    base = ev.inception_split_scores(x, r["w"], 128)
    x[128] *= 1e3
    huge = ev.inception_split_scores(x, r["w"], 128)
    alone = ev.inception_split_scores(x[:128], r["w"], 128)
    print(f"[huge row] splits {base} -> {huge}; the first 128 rows alone {alone}")
    assert base.shape == huge.shape == (2,) and alone.shape == (1,)
    assert huge[0] == base[0] == alone[0] and np.isfinite(huge[1]) and abs(huge[1] - 1.0) <= 1e-12 and abs(base[1] - 1.0) <= 1e-12


@pytest.mark.parametrize("index", [0, 1], ids=[ic.CASE_IDS[0], ic.CASE_IDS[1]])
def test_logits_stay_inside_their_buffer(index):
    """A guard row and guard columns around the n x C block keep their sentinel: rows >= n and columns >= C of the edge tiles are
    computed on the zero padding and not stored."""
    r = ic.reference(index)
    n, c = r["logits"].shape
    sentinel = -12345.5
    buf = torch.full((n + 1, c + 3), sentinel, device=DEV, dtype=torch.float32)
    out = ops.head_logits(_dev(r["x"]), _wt(r["w"]), buf[:n, :c])
    got = _np(buf)
    assert out.data_ptr() == buf.data_ptr()
    assert np.all(got[n] == sentinel) and np.all(got[:, c:] == sentinel)
    assert np.array_equal(got[:n, :c], _np(ops.head_logits(_dev(r["x"]), _wt(r["w"]))))
    lse, h = ops.is_rows(buf[:n, :c])                                  # the row pass reads a row-strided view as it is
    lse2, h2 = ops.is_rows(buf[:n, :c].contiguous())
    assert torch.equal(lse, lse2) and torch.equal(h, h2)


def test_non_finite_activations_are_refused():
    r = ic.reference(0)
    for bad in (np.nan, np.inf, -np.inf):
        x = r["x"].copy()
        x[17, 3] = bad
        with pytest.raises(ValueError, match="NaN or inf"):
            ev.compute_inception_score(x, r["w"])


def test_metrics_from_activations_with_and_without_a_weight():
    r = mc.reference(0)
    sp1, sp2 = mc.make_features(300, 260, 23, 9)
    w = ic.make_inputs(1, r["f2"].shape[1], 130, 5)[1]
    four = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2))
    five = ev.metrics_from_activations((r["f1"], sp1), (r["f2"], sp2), softmax_weight=w, split_size=100)
    direct = ev.compute_inception_score(r["f2"], w, split_size=100)
    ref = ic.score(ic.softmax64(r["f2"].astype(np.float64) @ w.astype(np.float64)), 100)
    print(f"[metrics] {five}; inception score direct {direct!r}, float64 restatement {ref!r}")
    assert sorted(four) == ["fid", "precision", "recall", "sfid"]
    assert sorted(five) == ["fid", "inception_score", "precision", "recall", "sfid"]
    assert five["inception_score"] == direct and isinstance(direct, float) and all(five[k] == four[k] for k in four)
    delta = float(ic.logit_tol(r["f2"], w).max())
    assert abs(np.log(direct) - np.log(ref)) <= ic.score_tol(delta, ic.softmax64(r["f2"].astype(np.float64) @ w.astype(np.float64)), 100)

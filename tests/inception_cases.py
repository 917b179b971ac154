"""Shared by test_inception_cpu.py and test_gpu_inception.py: the seeded inputs of the Inception-score tests and a float64 numpy
restatement of the reference's compute_inception_score (softmax(acts @ w), then exp(mean_i sum_c p (ln p - ln mean_i p)) per split,
averaged over the splits) with 0 * ln 0 := 0.  The restatement writes the formula as the reference does, p (ln p - ln m) summed per
row, not in the split form H - sum_c m ln m of the kernels, so it shares no rearrangement with the code under test.  Every reference
is computed once per process and must not be modified."""
import functools
import os

import numpy as np

import metrics_cases as mc

# (N, D, C, split_size, seed)
CASES = [
    (130, 23, 5, 64, 3),        # off every tile edge, odd D, ragged last split
    (257, 40, 130, 100, 5),     # C just past one column tile
    (300, 2023, 129, 128, 7),   # unaligned rows, splits on the row-tile edge
    (193, 2048, 1008, 5000, 9),  # the real head shape, one split
    (70, 8, 1, 32, 1),          # one class: every score is exactly 1
    (129, 16, 257, 1, 2),       # one-row splits: every score is 1
]
CASE_IDS = [f"{n}x{d}x{c}s{s}" for n, d, c, s, _ in CASES]
SCORED = (0, 1, 2, 3)           # the cases whose score is not 1 by construction

CHAIN = 3.5e-7                  # f32 MFMA chain up to K = 4096: |got - exact| <= CHAIN * sum_k |a_k b_k| (test_gpu_metrics.py)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inception_score.npz")


def make_inputs(n, d, c, seed):
    x = mc.make_features(n, 2, d, seed)[0]
    w = (np.random.default_rng(100 + seed).standard_normal((d, c)) * 3 / np.sqrt(d)).astype(np.float32)
    return x, w


def softmax64(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def kl_terms(part):
    """p (ln p - ln m) of one split, m the split's mean row; 0 where p = 0."""
    m = part.mean(0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(part > 0, np.log(part) - np.log(m), 0.0)
    return part * g


def split_scores(preds, split_size):
    """float64 [splits]: exp(mean_i sum_c p (ln p - ln m)) of every split of split_size rows, the last one ragged."""
    p = np.asarray(preds, np.float64)
    return np.array([np.exp(np.mean(np.sum(kl_terms(p[i:i + split_size]), 1))) for i in range(0, len(p), split_size)])


def score(preds, split_size):
    return float(np.mean(split_scores(preds, split_size)))


def mean_abs_terms(preds, split_size):
    """mean_i sum_c |p (ln p - ln m)| over all rows, m the marginal of each row's own split."""
    p = np.asarray(preds, np.float64)
    return float(np.concatenate([np.abs(kl_terms(p[i:i + split_size])).sum(1) for i in range(0, len(p), split_size)]).mean())


def logit_tol(x, w):
    """Per element: CHAIN * sum_k |x_ik w_kc|."""
    return CHAIN * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)))


def score_tol(delta, preds, split_size):
    """First-order propagation of a logit error delta: ln p = l - lse and ln m move by at most 2 delta each, so g = ln p - ln m by
    4 delta, and the weights p by a factor 1 +- 2 delta: |d ln score| <= 4 delta + 2 delta mean_i sum_c p |g|; 1 % for the second
    order."""
    return 1.01 * (4 * delta + 2 * delta * mean_abs_terms(preds, split_size))


def _freeze(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(index):
    """Everything the tests need of CASES[index], in float64, computed once."""
    n, d, c, split, seed = CASES[index]
    x, w = make_inputs(n, d, c, seed)
    logits = x.astype(np.float64) @ w.astype(np.float64)
    tol = logit_tol(x, w)
    p = softmax64(logits)
    return _freeze(dict(x=x, w=w, split=split, logits=logits, tol=tol, delta=float(tol.max()), preds=p, split_scores=split_scores(p, split),
                        score=score(p, split), score_tol=score_tol(float(tol.max()), p, split)))


@functools.lru_cache(maxsize=None)
def golden():
    """The fixture recorded from the reference (tests/golden/INCEPTION_SCORE.md): name -> dict of its arrays and scalars."""
    z = np.load(GOLDEN)
    out = {}
    for name in z["names"]:
        name = str(name)
        out[name] = _freeze(dict(acts=z[f"{name}_acts"], w=z[f"{name}_w"], preds=z[f"{name}_preds"], split=int(z[f"{name}_split"]),
                                 batch=int(z[f"{name}_batch"]), score_ref=float(z[f"{name}_score_ref"]), score_f64=float(z[f"{name}_score_f64"])))
    return out, float(z["max_rel_gap"])

#!/usr/bin/env python3
"""Generate tests/golden/inception_score.npz by running the UNMODIFIED reference's `Evaluator.compute_inception_score`
(evaluations/evaluator.py) on the host:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_inception_goldens.py <reference checkout>

The reference module imports TensorFlow and requests at the top; empty stub modules stand in for them (and for tqdm where it is
absent), exactly as in make_metrics_goldens.py.  The evaluator object is made with `Evaluator.__new__` (its constructor builds the
TensorFlow graph) and given what the method reads: `softmax_batch_size`, placeholder objects for `softmax` / `softmax_input`, and a
fake `sess` whose `run` returns the float32 numpy softmax(acts @ w) of the batch it is fed -- what the softmax graph computes.  The
batching, the concatenation and the score arithmetic that run are the reference's own.  Only data is written.

Per case: the inputs, the `preds` the fake session returned (in feed order, i.e. row order), `score_ref` (what the reference
returned: float32 numpy arithmetic) and `score_f64` (this script's float64 evaluation of the same formula on the same `preds`, with
0 * ln 0 := 0).  The case `zero` scales the weight until the float32 softmax underflows to exact zeros: the reference returns NaN
there and NaN is what is stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_metrics_goldens import install_stubs  # noqa: E402

# name, rows, width, classes, split_size, softmax_batch_size, weight scale, seed
CASES = [
    ("s16_b5", 37, 12, 7, 16, 5, 1.0, 21),
    ("s37_b512", 37, 12, 7, 37, 512, 1.0, 22),
    ("s5000_b5", 37, 12, 7, 5000, 5, 1.0, 23),
    ("s16_b512", 37, 12, 7, 16, 512, 1.0, 24),
    ("zero", 37, 12, 7, 16, 5, 60.0, 25),
]


def inputs(n, d, c, scale, seed):
    rng = np.random.default_rng(seed)
    acts = np.maximum(rng.standard_normal((n, d)) + 0.5, 0).astype(np.float32)
    w = (rng.standard_normal((d, c)) * scale * 3 / np.sqrt(d)).astype(np.float32)
    return acts, w


class FakeSession:
    """sess.run(softmax, {softmax_input: acts}) -> float32 softmax(acts @ w), and a record of what it returned."""

    def __init__(self, w):
        self.w = w
        self.returned = []

    def run(self, fetch, feed_dict):
        (acts,) = feed_dict.values()
        logits = np.asarray(acts, np.float32) @ self.w
        e = np.exp(logits - logits.max(1, keepdims=True))
        out = (e / e.sum(1, keepdims=True)).astype(np.float32)
        self.returned.append(out)
        return out


def score_f64(preds, split_size):
    p = np.asarray(preds, np.float64)
    scores = []
    for i in range(0, len(p), split_size):
        part = p[i:i + split_size]
        m = part.mean(0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(part > 0, np.log(part) - np.log(m), 0.0)
        scores.append(np.exp(np.mean(np.sum(part * g, 1))))
    return float(np.mean(scores))


def main():
    ref = sys.argv[1]
    install_stubs()
    sys.path.insert(0, ref)
    from evaluations import evaluator as E
    out = {"names": np.array([c[0] for c in CASES])}
    worst = 0.0
    for name, n, d, c, split, batch, scale, seed in CASES:
        acts, w = inputs(n, d, c, scale, seed)
        ev = E.Evaluator.__new__(E.Evaluator)
        ev.softmax_batch_size = batch
        ev.softmax, ev.softmax_input = object(), object()
        ev.sess = FakeSession(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            got = ev.compute_inception_score(acts, split_size=split)
        preds = np.concatenate(ev.sess.returned, 0)
        assert preds.dtype == np.float32 and preds.shape == (n, c) and len(ev.sess.returned) == -(-n // batch)
        f64 = score_f64(preds, split)
        zeros = int((preds == 0).sum())
        if name == "zero":
            assert zeros > 0 and np.isnan(got) and np.isfinite(f64)
        else:
            assert zeros == 0 and np.isfinite(got)
            worst = max(worst, abs(got - f64) / f64)
        print(f"{name}: score_ref {got!r} score_f64 {f64!r} zeros {zeros} rel gap {abs(got - f64) / f64:.3e}")
        out.update({f"{name}_acts": acts, f"{name}_w": w, f"{name}_preds": preds, f"{name}_split": np.int64(split),
                    f"{name}_batch": np.int64(batch), f"{name}_score_ref": np.float64(got), f"{name}_score_f64": np.float64(f64)})
    out["max_rel_gap"] = np.float64(worst)
    print(f"largest |score_ref - score_f64| / score_f64 over the finite cases: {worst:.3e}")
    np.savez(os.path.join(HERE, "inception_score.npz"), **out)


if __name__ == "__main__":
    main()

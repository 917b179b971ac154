#!/usr/bin/env python3
"""Generate tests/golden/metrics_fid.npz by running the UNMODIFIED reference's FID arithmetic on the host:
`Evaluator.compute_statistics` and `FIDStatistics.frechet_distance` of evaluations/evaluator.py.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_metrics_goldens.py <reference checkout>

The reference module imports TensorFlow and requests at the top; neither is needed by the two functions recorded here, so empty
stub modules stand in for them (and for tqdm where it is absent).  Only numpy and scipy code of the reference runs.  Only data is
written: the statistics of the seeded inputs, the distances and which branch of frechet_distance was taken."""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def install_stubs():
    names = ["tensorflow", "tensorflow._api", "tensorflow._api.v2", "tensorflow._api.v2.compat", "tensorflow._api.v2.compat.v1",
             "tensorflow.compat", "tensorflow.compat.v1", "requests"]
    try:
        import tqdm.auto  # noqa: F401
    except ImportError:
        names += ["tqdm", "tqdm.auto"]
    for name in names:
        mod = sys.modules.setdefault(name, types.ModuleType(name))
        if "." in name:
            parent, leaf = name.rsplit(".", 1)
            setattr(sys.modules[parent], leaf, mod)
    if "tqdm.auto" in names:
        sys.modules["tqdm.auto"].tqdm = lambda it, *a, **k: it


def pair(kind):
    """Two activation sets.  'well': [200, 24], full-rank covariances.  'singular': [12, 24], N < D, so both covariances have rank
    11 and their product is singular."""
    rng = np.random.default_rng({"well": 11, "singular": 12}[kind])
    n = 200 if kind == "well" else 12
    mix_a, mix_b = rng.standard_normal((24, 24)) / 5 + np.eye(24), rng.standard_normal((24, 24)) / 5 + np.eye(24)
    a = np.maximum(rng.standard_normal((n, 24)) @ mix_a + 1.0, 0)
    b = np.maximum(0.8 * rng.standard_normal((n, 24)) @ mix_b + 1.3, 0)
    return a, b


def main():
    ref = sys.argv[1]
    install_stubs()
    sys.path.insert(0, ref)
    from evaluations import evaluator as E
    out = {}
    for kind in ("well", "singular"):
        a, b = pair(kind)
        sa, sb = E.Evaluator.compute_statistics(None, a), E.Evaluator.compute_statistics(None, b)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fd = sa.frechet_distance(sb)
        eps_branch = any("singular product" in str(w.message) for w in caught)
        assert np.isfinite(fd)
        out.update({f"{kind}_mu_a": sa.mu, f"{kind}_sigma_a": sa.sigma, f"{kind}_mu_b": sb.mu,
                    f"{kind}_sigma_b": sb.sigma, f"{kind}_fd": np.float64(fd), f"{kind}_fd_rev": np.float64(sb.frechet_distance(sa)),
                    f"{kind}_eps_branch": np.bool_(eps_branch)})
        print(kind, "fd", fd, "eps branch", eps_branch)
    np.savez(os.path.join(HERE, "metrics_fid.npz"), **out)


if __name__ == "__main__":
    main()

"""FID statistics, Frechet distance, precision / recall, the Inception score, KID and density / coverage from Inception activations: the part of the
reference's evaluations/evaluator.py that follows `compute_activations`, with the reference's names and return types and no
TensorFlow.

The all-pairs distance work of `ManifoldEstimator`, the float64 mean / covariance of `compute_statistics` and the whole of
`compute_inception_score` -- the head product pool activations x softmax weight, the row softmax, the per-split entropies and class
marginals -- run as HIP kernels (csrc/metrics.hip); percentile clamping, the means of the flags, the mean over the splits and the
matrix square root of the Frechet distance stay on the host in numpy / scipy as the reference has them.  Inputs are numpy arrays or
torch tensors, on the CPU or on the device; they are uploaded once as float32 and a contiguous float32 device tensor is used in place.

The Inception score needs one array from the user: the `[2048, 1008]` operand of the graph's `softmax/logits/MatMul` (there is no
bias), as an array or a `.npy` / `.npz` path (INTEGRATION.md says how to get it out of the graph file offline).

Deliberate differences.  (1) The reference computes distances in fp16 and falls back to f32 only when that overflows, so its radii
and comparisons are quantised to fp16 (about 0.25 at typical pool-feature distances).  Here every distance is f32:
max((|u|^2 - 2 u.v) + |v|^2, 0) with the dot product an ordered f32 fma chain.  Precision and recall can differ from a TensorFlow
run in the third decimal.  (2) The reference reduces the Inception score in float32 numpy and computes 0 * log 0 = NaN once a
float32 softmax underflows (a logit about 104 below its row's maximum): the whole score is then NaN.  Here the softmax and both
sums are float64 and a term with p = 0 or a class marginal of 0 is its limit 0, so the score stays finite.

Beside the reference's metrics: the kernel inception distance (`polynomial_mmd2`, `kid_subset_scores`, `compute_kid`: the unbiased
polynomial-kernel MMD^2 of Binkowski et al. 2018, float64 row sums in a fixed order from one launch per kernel matrix, the subsets
read through index tables) and density / coverage (`ManifoldEstimator.evaluate_dc`, `compute_density_coverage`: Naeem et al. 2020,
counts and flags under the same radii, compared with `<` where precision / recall keep the reference's `<=`).

Not built: the Inception feature extractor (`compute_activations` / `read_activations`: its weights are a download) and
`ManifoldEstimator.evaluate` (realism scores)."""
import os
import warnings

import numpy as np
import torch

from . import ops


class InvalidFIDException(Exception):
    pass


def _sqrtm(a):
    from scipy import linalg          # lazy: only the Frechet distance needs scipy
    try:
        out = linalg.sqrtm(a, disp=False)
    except TypeError:                 # a scipy without the keyword
        out = linalg.sqrtm(a)
    return out[0] if isinstance(out, tuple) else out


class FIDStatistics:
    def __init__(self, mu, sigma):
        self.mu = mu
        self.sigma = sigma

    def frechet_distance(self, other, eps=1e-6):
        """|mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2)) in host float64; a non-finite square root is retried with eps
        added to both diagonals (with a warning), a complex one is accepted when its diagonal is real to 1e-3."""
        mu1, mu2 = np.atleast_1d(self.mu), np.atleast_1d(other.mu)
        sigma1, sigma2 = np.atleast_2d(self.sigma), np.atleast_2d(other.sigma)
        assert mu1.shape == mu2.shape, f"Training and test mean vectors have different lengths: {mu1.shape}, {mu2.shape}"
        assert sigma1.shape == sigma2.shape, f"Training and test covariances have different dimensions: {sigma1.shape}, {sigma2.shape}"
        diff = mu1 - mu2
        covmean = _sqrtm(sigma1.dot(sigma2))
        if not np.isfinite(covmean).all():
            warnings.warn("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
            offset = np.eye(sigma1.shape[0]) * eps
            covmean = _sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if np.iscomplexobj(covmean):
            if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
                raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
            covmean = covmean.real
        return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def _as_tensor(x, what):
    """The input as a torch tensor where it lies, refused unless it is non-empty and 2-D (checked before anything is uploaded)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x)) if x.flags.writeable else torch.tensor(x)      # torch warns on read-only arrays
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}: expected a numpy array or a torch tensor, got {type(x).__name__}")
    if x.dim() != 2:
        raise ValueError(f"{what}: expected 2-D [N, D] activations, got shape {tuple(x.shape)}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: empty activations of shape {tuple(x.shape)}")
    return x


def _same_width(what, a, b):
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: feature widths differ: {a.shape[1]} and {b.shape[1]}")


def _device_features(x, what):
    """float32 contiguous [N, D] on the GPU: one upload for host data, the tensor itself where it already is that."""
    x = _as_tensor(x, what)
    if not x.is_cuda:
        x = x.to(torch.float32).cuda()       # no GPU: torch raises here, there is no host path
    return x.to(torch.float32).contiguous()


def _norms(x, what):
    """Row square norms, and the one device reduction that refuses NaN / inf features (a non-finite feature, or a row whose
    square norm overflows f32, makes its norm non-finite)."""
    n = ops.row_sqnorms(x)
    if not bool(torch.isfinite(n).all()):
        raise ValueError(f"{what}: features hold NaN or inf (or a row's square norm overflows float32)")
    return n


def compute_statistics(activations):
    """FIDStatistics(mu, sigma) of [N, D] activations: numpy float64 mean and covariance (np.cov(rowvar=False)), two kernels."""
    x = _device_features(activations, "compute_statistics")
    mu = ops.col_mean_f64(x)
    if not bool(torch.isfinite(mu).all()):
        raise ValueError("compute_statistics: activations hold NaN or inf")
    sigma = ops.cov_f64(x, mu)
    return FIDStatistics(mu.cpu().numpy(), sigma.cpu().numpy())


class ManifoldEstimator:
    """k-nearest-neighbour manifolds of feature sets (improved precision and recall).  The reference's constructor without its
    TensorFlow session.  `row_batch_size` / `col_batch_size` cut the work into launches; no output bit depends on them."""

    def __init__(self, row_batch_size=10000, col_batch_size=10000, nhood_sizes=(3,), clamp_to_percentile=None, eps=1e-5):
        if row_batch_size < 1 or col_batch_size < 1:
            raise ValueError(f"ManifoldEstimator: batch sizes must be positive, got {row_batch_size} x {col_batch_size}")
        nhood_sizes = tuple(int(k) for k in nhood_sizes)
        if not nhood_sizes or min(nhood_sizes) < 0 or max(nhood_sizes) + 1 > ops.KSMALLEST_MAX:
            raise ValueError(f"ManifoldEstimator: nhood_sizes {nhood_sizes} outside 0 .. {ops.KSMALLEST_MAX - 1}")
        if len(nhood_sizes) > ops.WITHIN_MAX_RADII:
            raise ValueError(f"ManifoldEstimator: at most {ops.WITHIN_MAX_RADII} neighbourhood sizes, got {len(nhood_sizes)}")
        self.row_batch_size = int(row_batch_size)
        self.col_batch_size = int(col_batch_size)
        self.nhood_sizes = nhood_sizes
        self.num_nhoods = len(nhood_sizes)
        self.clamp_to_percentile = clamp_to_percentile
        self.eps = eps

    def _ksmallest(self, x, norms, k1):
        """[N, k1] ascending smallest distances of every row of x to all rows of x (itself included), cut into launches."""
        n = x.shape[0]
        out = torch.empty(n, k1, device=x.device, dtype=torch.float32)
        cols = [(c0, min(c0 + self.col_batch_size, n)) for c0 in range(0, n, self.col_batch_size)]
        for r0 in range(0, n, self.row_batch_size):
            r1 = min(r0 + self.row_batch_size, n)
            if len(cols) == 1:
                out[r0:r1] = ops.pairwise_ksmallest(x[r0:r1], x, k1, norms[r0:r1], norms)
                continue
            parts = torch.full((len(cols), r1 - r0, k1), float("inf"), device=x.device, dtype=torch.float32)
            for ci, (c0, c1) in enumerate(cols):
                kc = min(k1, c1 - c0)
                parts[ci, :, :kc] = ops.pairwise_ksmallest(x[r0:r1], x[c0:c1], kc, norms[r0:r1], norms[c0:c1])
            out[r0:r1] = ops.ksmallest_merge(parts)
        return out

    def manifold_radii(self, features):
        """float32 [N, len(nhood_sizes)]: the distance of every point to its k-th nearest neighbour, itself counted as the 0-th."""
        features = _as_tensor(features, "manifold_radii")
        kmax = max(self.nhood_sizes)
        if features.shape[0] <= kmax:
            raise ValueError(f"manifold_radii: N = {features.shape[0]} points, more than max(nhood_sizes) = {kmax} are needed")
        x = _device_features(features, "manifold_radii")
        norms = _norms(x, "manifold_radii")
        small = self._ksmallest(x, norms, kmax + 1)
        radii = np.ascontiguousarray(small.cpu().numpy()[:, list(self.nhood_sizes)], dtype=np.float32)
        if self.clamp_to_percentile is not None:
            max_distances = np.percentile(radii, self.clamp_to_percentile, axis=0)
            radii[radii > max_distances] = 0
        return radii

    def evaluate(self, features, radii, eval_features):
        raise NotImplementedError("ManifoldEstimator.evaluate (realism scores) is not built on the HIP path; evaluate_pr is")

    def evaluate_pr(self, features_1, radii_1, features_2, radii_2):
        """(precision [K1], recall [K2]) as float64 means: precision[c] is the share of features_2 within radii_1[:, c] of some
        point of features_1, recall[c] the share of features_1 within radii_2[:, c] of some point of features_2."""
        features_1, features_2 = _as_tensor(features_1, "evaluate_pr"), _as_tensor(features_2, "evaluate_pr")
        _same_width("evaluate_pr", features_1, features_2)
        r1, r2 = (torch.as_tensor(np.asarray(r), dtype=torch.float32) for r in (radii_1, radii_2))
        for r, x, name in ((r1, features_1, "radii_1"), (r2, features_2, "radii_2")):
            if r.dim() != 2 or r.shape[0] != x.shape[0] or not 1 <= r.shape[1] <= ops.WITHIN_MAX_RADII:
                raise ValueError(f"evaluate_pr: {name} must be [{x.shape[0]}, 1 .. {ops.WITHIN_MAX_RADII}], got {tuple(r.shape)}")
        x1, x2 = _device_features(features_1, "evaluate_pr"), _device_features(features_2, "evaluate_pr")
        r1, r2 = r1.to(x1.device).contiguous(), r2.to(x1.device).contiguous()
        n1, n2 = _norms(x1, "evaluate_pr"), _norms(x2, "evaluate_pr")
        status_1 = torch.zeros(x1.shape[0], r2.shape[1], device=x1.device, dtype=torch.uint8)
        status_2 = torch.zeros(x2.shape[0], r1.shape[1], device=x1.device, dtype=torch.uint8)
        for b1 in range(0, x1.shape[0], self.row_batch_size):
            e1 = min(b1 + self.row_batch_size, x1.shape[0])
            for b2 in range(0, x2.shape[0], self.col_batch_size):
                e2 = min(b2 + self.col_batch_size, x2.shape[0])
                ops.pairwise_within(x1[b1:e1], x2[b2:e2], n1[b1:e1], n2[b2:e2], r1[b1:e1], r2[b2:e2], status_1[b1:e1], status_2[b2:e2])
        self.last_status = (status_1.cpu().numpy().astype(bool), status_2.cpu().numpy().astype(bool))
        return (np.mean(self.last_status[1].astype(np.float64), axis=0), np.mean(self.last_status[0].astype(np.float64), axis=0))

    def evaluate_dc(self, features_real, radii_real, features_fake):
        """(density [K], coverage [K]) as float64 (Naeem et al. 2020): density[c] is the number of pairs (fake i, real j) with
        d(i, j) < radii_real[j, c], over nhood_sizes[c] times the number of fake points; coverage[c] the share of real points with a
        fake point strictly inside radii_real[:, c].  Strictly below, where evaluate_pr takes <=.  The counts [M, K] and the flags
        [N, K] stay in last_counts / last_covered."""
        features_real, features_fake = _as_tensor(features_real, "evaluate_dc"), _as_tensor(features_fake, "evaluate_dc")
        _same_width("evaluate_dc", features_real, features_fake)
        r = torch.tensor(np.asarray(radii_real, dtype=np.float32))         # a copy: torch warns on read-only arrays
        if r.dim() != 2 or tuple(r.shape) != (features_real.shape[0], self.num_nhoods):
            raise ValueError(f"evaluate_dc: radii_real must be [{features_real.shape[0]}, {self.num_nhoods}], got {tuple(r.shape)}")
        if min(self.nhood_sizes) < 1:
            raise ValueError(f"evaluate_dc: density divides by the neighbourhood size, nhood_sizes {self.nhood_sizes} holds 0")
        real, fake = _device_features(features_real, "evaluate_dc"), _device_features(features_fake, "evaluate_dc")
        r = r.to(real.device).contiguous()
        n_real, n_fake = _norms(real, "evaluate_dc"), _norms(fake, "evaluate_dc")
        counts = torch.zeros(fake.shape[0], r.shape[1], device=real.device, dtype=torch.int32)
        covered = torch.zeros(real.shape[0], r.shape[1], device=real.device, dtype=torch.uint8)
        for b1 in range(0, fake.shape[0], self.row_batch_size):
            e1 = min(b1 + self.row_batch_size, fake.shape[0])
            for b2 in range(0, real.shape[0], self.col_batch_size):
                e2 = min(b2 + self.col_batch_size, real.shape[0])
                ops.pairwise_count_within(fake[b1:e1], real[b2:e2], n_fake[b1:e1], n_real[b2:e2], r[b2:e2], counts[b1:e1], covered[b2:e2])
        self.last_counts, self.last_covered = counts.cpu().numpy(), covered.cpu().numpy().astype(bool)
        density = self.last_counts.sum(0, dtype=np.int64) / (np.asarray(self.nhood_sizes, np.float64) * fake.shape[0])
        return (density, np.mean(self.last_covered.astype(np.float64), axis=0))


def _dc_args(what, activations_ref, activations_sample, nearest_k):
    """The argument checks of compute_density_coverage, made before anything is uploaded."""
    ref, sample = _as_tensor(activations_ref, what), _as_tensor(activations_sample, what)
    _same_width(what, ref, sample)
    if isinstance(nearest_k, bool) or int(nearest_k) != nearest_k or not 1 <= nearest_k < ops.KSMALLEST_MAX:
        raise ValueError(f"{what}: nearest_k must be an integer in 1 .. {ops.KSMALLEST_MAX - 1}, got {nearest_k}")
    if ref.shape[0] <= nearest_k:
        raise ValueError(f"{what}: N = {ref.shape[0]} reference points, more than nearest_k = {nearest_k} are needed")
    return ref, sample, int(nearest_k)


def compute_density_coverage(activations_ref, activations_sample, nearest_k=5, manifold_estimator=None):
    """(density, coverage) of the sample set against the reference set (Naeem et al. 2020) with the radii of the reference set's
    nearest_k-th neighbours, itself counted as the 0-th.  A given estimator lends its batch sizes and clamping; the neighbourhood
    size is nearest_k."""
    ref, sample, nearest_k = _dc_args("compute_density_coverage", activations_ref, activations_sample, nearest_k)
    src = manifold_estimator or ManifoldEstimator()
    est = ManifoldEstimator(src.row_batch_size, src.col_batch_size, (nearest_k,), src.clamp_to_percentile, src.eps)
    ref, sample = _device_features(ref, "compute_density_coverage"), _device_features(sample, "compute_density_coverage")
    density, coverage = est.evaluate_dc(ref, est.manifold_radii(ref), sample)
    return (float(density[0]), float(coverage[0]))


KID_WORKSPACE_BYTES = 64 << 20    # most partial-sum workspace of one pairwise_polysum launch: caps the subsets per launch
POLYSUM_MAX_ROWS = 65536          # rows of a full set per pairwise_polysum launch


def _kernel_args(what, width, degree, gamma, coef0):
    if isinstance(degree, bool) or int(degree) != degree or not 1 <= degree <= ops.POLYSUM_MAX_DEGREE:
        raise ValueError(f"{what}: degree must be an integer in 1 .. {ops.POLYSUM_MAX_DEGREE}, got {degree}")
    gamma = 1.0 / width if gamma is None else float(gamma)
    if not (np.isfinite(gamma) and np.isfinite(coef0)):
        raise ValueError(f"{what}: gamma = {gamma} and coef0 = {coef0} must be finite")
    return int(degree), gamma, float(coef0)


def _ordered_sum(a, axis=-1):
    """The float64 sum along an axis, added strictly in index order (np.sum adds pairwise)."""
    return np.take(np.cumsum(a, axis=axis, dtype=np.float64), -1, axis=axis)


def _mmd2(sxx, syy, sxy, m, n):
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2 * sxy / (m * n)


def polynomial_mmd2(x, y, degree=3, gamma=None, coef0=1.0):
    """The unbiased MMD^2 of the kernel k(a, b) = (gamma a.b + coef0)^degree between the full sets x [m, D] and y [n, D]:
    sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n).  gamma None is
    1 / D.  The sets are cut into launches along the rows only, so a row's sum keeps its order; the three totals are the float64 row
    sums added in row order on the host."""
    what = "polynomial_mmd2"
    x, y = _as_tensor(x, what), _as_tensor(y, what)
    _same_width(what, x, y)
    degree, gamma, coef0 = _kernel_args(what, x.shape[1], degree, gamma, coef0)
    if min(x.shape[0], y.shape[0]) < 2:
        raise ValueError(f"{what}: {x.shape[0]} and {y.shape[0]} points, at least 2 are needed in each set")
    x, y = _device_features(x, what), _device_features(y, what)
    _norms(x, what), _norms(y, what)

    def total(u, v, skip):
        sums = []
        for r0 in range(0, u.shape[0], POLYSUM_MAX_ROWS):
            r1 = min(r0 + POLYSUM_MAX_ROWS, u.shape[0])
            rows = torch.arange(r0, r1, dtype=torch.int32, device=u.device)[None] if skip and (r0 or r1 < u.shape[0]) else None
            sums.append(ops.pairwise_polysum(u if rows is not None else u[r0:r1], v, gamma, coef0, degree, u_idx=rows, skip_diagonal=skip)[0])
        return float(_ordered_sum(torch.cat(sums).cpu().numpy()))

    return float(_mmd2(total(x, x, True), total(y, y, True), total(x, y, False), x.shape[0], y.shape[0]))


def _kid_args(what, activations_ref, activations_sample, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0):
    """The argument checks of kid_subset_scores, made before anything is uploaded."""
    ref, sample = _as_tensor(activations_ref, what), _as_tensor(activations_sample, what)
    _same_width(what, ref, sample)
    degree, gamma, coef0 = _kernel_args(what, ref.shape[1], degree, gamma, coef0)
    if isinstance(num_subsets, bool) or int(num_subsets) != num_subsets or num_subsets < 1:
        raise ValueError(f"{what}: num_subsets must be a positive integer, got {num_subsets}")
    if isinstance(subset_size, bool) or int(subset_size) != subset_size or not 2 <= subset_size <= min(ref.shape[0], sample.shape[0]):
        raise ValueError(f"{what}: subset_size = {subset_size} outside 2 .. min(N) = {min(ref.shape[0], sample.shape[0])}")
    np.random.RandomState(seed)          # refuses a seed numpy cannot take
    return ref, sample, int(num_subsets), int(subset_size), degree, gamma, coef0


def kid_subset_indices(n_ref, n_sample, num_subsets=100, subset_size=1000, seed=0):
    """(ref_idx, sample_idx), int32 [num_subsets, subset_size]: rng = np.random.RandomState(seed), and per subset first
    rng.choice(n_ref, subset_size, replace=False), then rng.choice(n_sample, subset_size, replace=False)."""
    rng = np.random.RandomState(seed)
    ref_idx = np.empty((num_subsets, subset_size), np.int32)
    sample_idx = np.empty((num_subsets, subset_size), np.int32)
    for s in range(num_subsets):
        ref_idx[s] = rng.choice(n_ref, subset_size, replace=False)
        sample_idx[s] = rng.choice(n_sample, subset_size, replace=False)
    return ref_idx, sample_idx


def kid_subset_scores(activations_ref, activations_sample, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0):
    """float64 [num_subsets]: the unbiased polynomial-kernel MMD^2 between a random subset of subset_size reference activations and
    one of subset_size sample activations, drawn as kid_subset_indices draws them.  All subsets go to the device as two index tables;
    a batch of subsets is three pairwise_polysum launches and no activation is copied."""
    what = "kid_subset_scores"
    ref, sample, num_subsets, m, degree, gamma, coef0 = _kid_args(what, activations_ref, activations_sample, num_subsets, subset_size, degree,
                                                                  gamma, coef0, seed)
    ref_idx, sample_idx = kid_subset_indices(ref.shape[0], sample.shape[0], num_subsets, m, seed)
    ref, sample = _device_features(ref, what), _device_features(sample, what)
    _norms(ref, what), _norms(sample, what)
    per_launch = max(1, KID_WORKSPACE_BYTES // (m * 2 * 16 * 8))        # a row has at most 2 * 16 float64 partial sums
    scores = np.empty(num_subsets, np.float64)
    for b0 in range(0, num_subsets, per_launch):
        ri, si = ref_idx[b0:b0 + per_launch], sample_idx[b0:b0 + per_launch]
        sxx, syy, sxy = (_ordered_sum(ops.pairwise_polysum(u, v, gamma, coef0, degree, ui, vi, skip).cpu().numpy())
                         for u, v, ui, vi, skip in ((ref, ref, ri, ri, True), (sample, sample, si, si, True), (ref, sample, ri, si, False)))
        scores[b0:b0 + per_launch] = _mmd2(sxx, syy, sxy, m, m)
    return scores


def compute_kid(activations_ref, activations_sample, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0):
    """(mean, std): the kernel inception distance of Binkowski et al. 2018 as the numpy mean and std (ddof 0) of kid_subset_scores."""
    scores = kid_subset_scores(activations_ref, activations_sample, num_subsets, subset_size, degree, gamma, coef0, seed)
    return (float(np.mean(scores)), float(np.std(scores)))


def compute_prec_recall(activations_ref, activations_sample, manifold_estimator=None):
    """(precision, recall) of the sample set against the reference set, neighbourhood size nhood_sizes[0]."""
    est = manifold_estimator or ManifoldEstimator()
    activations_ref, activations_sample = _as_tensor(activations_ref, "compute_prec_recall"), _as_tensor(activations_sample, "compute_prec_recall")
    _same_width("compute_prec_recall", activations_ref, activations_sample)
    if min(activations_ref.shape[0], activations_sample.shape[0]) <= max(est.nhood_sizes):
        raise ValueError(f"compute_prec_recall: N = {activations_ref.shape[0]} and {activations_sample.shape[0]} points, more than "
                         f"max(nhood_sizes) = {max(est.nhood_sizes)} are needed in each set")
    ref = _device_features(activations_ref, "compute_prec_recall")
    sample = _device_features(activations_sample, "compute_prec_recall")
    radii_1 = est.manifold_radii(ref)
    radii_2 = est.manifold_radii(sample)
    pr = est.evaluate_pr(ref, radii_1, sample, radii_2)
    return (float(pr[0][0]), float(pr[1][0]))


MAX_SOFTMAX_ROWS = 65536      # rows per launch when softmax_batch_size is None: 264 MB of logits at C = 1008


class _SoftmaxHead:
    """The [D, C] softmax weight, checked where it lies; its class-major [C, D] device copy is made on first use and kept."""

    def __init__(self, softmax_weight, what="compute_inception_score"):
        w = softmax_weight
        if isinstance(w, (str, os.PathLike)):
            w = np.load(w)
            if isinstance(w, np.lib.npyio.NpzFile):
                if "softmax_weight" not in w.files:
                    raise ValueError(f"{what}: {softmax_weight} has no array named softmax_weight (it holds {w.files})")
                w = w["softmax_weight"]
        if isinstance(w, np.ndarray):
            w = torch.from_numpy(np.ascontiguousarray(w)) if w.flags.writeable else torch.tensor(w)
        if not isinstance(w, torch.Tensor):
            raise ValueError(f"{what}: softmax_weight must be a numpy array, a torch tensor or a .npy / .npz path, got {type(w).__name__}")
        if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1:
            raise ValueError(f"{what}: softmax_weight must be 2-D [D, C], got shape {tuple(w.shape)}")
        if not w.is_floating_point() or not bool(torch.isfinite(w).all()):
            raise ValueError(f"{what}: softmax_weight must be floating point without NaN or inf")
        self.weight = w
        self.width, self.classes = w.shape
        self._wt = None

    def class_major(self):
        if self._wt is None:
            w = self.weight if self.weight.is_cuda else self.weight.to(torch.float32).cuda()
            self._wt = w.to(torch.float32).t().contiguous()
        return self._wt


def _split_size(what, split_size):
    if int(split_size) != split_size or split_size < 1:
        raise ValueError(f"{what}: split_size must be a positive integer, got {split_size}")
    return int(split_size)


def _batch_rows(what, softmax_batch_size):
    if softmax_batch_size is None:
        return MAX_SOFTMAX_ROWS
    if int(softmax_batch_size) != softmax_batch_size or softmax_batch_size < 1:
        raise ValueError(f"{what}: softmax_batch_size must be a positive integer or None, got {softmax_batch_size}")
    return int(softmax_batch_size)


def _finite_scores(what, scores):
    scores = scores.cpu().numpy()
    if not np.isfinite(scores).all():
        raise ValueError(f"{what}: a split's score is not finite (logits or probabilities beyond float32 / float64 range)")
    return scores


def inception_split_scores(activations, softmax_weight, split_size=5000, softmax_batch_size=None, what="inception_split_scores"):
    """float64 [splits]: exp(mean_i sum_c p_ic (ln p_ic - ln mean_i p_ic)) of every split of split_size rows (the last one ragged),
    p = softmax(activations @ softmax_weight).  compute_inception_score is the mean of these."""
    head = softmax_weight if isinstance(softmax_weight, _SoftmaxHead) else _SoftmaxHead(softmax_weight, what)
    acts = _as_tensor(activations, what)
    if acts.shape[1] != head.width:
        raise ValueError(f"{what}: activations are {acts.shape[1]} wide, softmax_weight is [{head.width}, {head.classes}]")
    split, batch = _split_size(what, split_size), _batch_rows(what, softmax_batch_size)
    x = _device_features(acts, what)
    _norms(x, what)
    wt = head.class_major()
    n, C = x.shape[0], head.classes
    split, batch = min(split, n), min(batch, n)
    lse = torch.empty(n, device=x.device, dtype=torch.float64)
    h = torch.empty(n, device=x.device, dtype=torch.float64)
    colsum = torch.zeros(-(-n // split), C, device=x.device, dtype=torch.float64)
    logits = torch.empty(batch, C, device=x.device, dtype=torch.float32)
    for r0 in range(0, n, batch):
        r1 = min(r0 + batch, n)
        rows = ops.head_logits(x[r0:r1], wt, logits[:r1 - r0])
        ops.is_rows(rows, False, lse[r0:r1], h[r0:r1])
        ops.is_colsums(rows, lse[r0:r1], r0, split, colsum)
    return _finite_scores(what, ops.is_finish(h, colsum, split))


def compute_inception_score(activations, softmax_weight, split_size=5000, softmax_batch_size=None):
    """The reference's Evaluator.compute_inception_score: the mean over the splits of inception_split_scores.  activations: [N, D]
    pool activations; softmax_weight: the [D, C] weight of the reference's softmax graph (an array or a .npy / .npz path);
    softmax_batch_size caps the rows per launch and so the logits buffer, and no output bit depends on it."""
    return float(np.mean(inception_split_scores(activations, softmax_weight, split_size, softmax_batch_size, "compute_inception_score")))


def inception_split_scores_from_probs(preds, split_size=5000, what="inception_split_scores_from_probs"):
    """inception_split_scores on given [N, C] probabilities (rows need not sum to 1)."""
    p = _as_tensor(preds, what)
    split = _split_size(what, split_size)
    if not bool(torch.isfinite(p).all()) or bool((p < 0).any()):
        raise ValueError(f"{what}: probabilities must be finite and non-negative")
    p = _device_features(p, what)
    n, C = p.shape
    split = min(split, n)
    colsum = torch.zeros(-(-n // split), C, device=p.device, dtype=torch.float64)
    h = torch.empty(n, device=p.device, dtype=torch.float64)
    for r0 in range(0, n, MAX_SOFTMAX_ROWS):
        rows = p[r0:r0 + MAX_SOFTMAX_ROWS]
        ops.is_rows(rows, True, None, h[r0:r0 + MAX_SOFTMAX_ROWS])
        ops.is_colsums(rows, None, r0, split, colsum, probs=True)
    return _finite_scores(what, ops.is_finish(h, colsum, split))


def inception_score_from_probs(preds, split_size=5000):
    """The second half of the reference's compute_inception_score on given [N, C] probabilities (rows need not sum to 1)."""
    return float(np.mean(inception_split_scores_from_probs(preds, split_size, "inception_score_from_probs")))


class Evaluator:
    """The reference's Evaluator without its TensorFlow session: what follows compute_activations.  softmax_weight is the [D, C]
    matrix of the Inception graph's softmax head (array or .npy / .npz path), needed by compute_inception_score only."""

    def __init__(self, softmax_weight=None, manifold_estimator=None, softmax_batch_size=None):
        self.softmax_batch_size = None if softmax_batch_size is None else _batch_rows("Evaluator", softmax_batch_size)
        self.manifold_estimator = manifold_estimator or ManifoldEstimator()
        self.softmax_head = None if softmax_weight is None else _SoftmaxHead(softmax_weight, "Evaluator")

    def compute_activations(self, batches):
        raise NotImplementedError("Evaluator.compute_activations: the Inception feature extractor is not built on the HIP path "
                                  "(its weights are a download); start from pool / spatial activations")

    def read_activations(self, npz_path):
        raise NotImplementedError("Evaluator.read_activations: the Inception feature extractor is not built on the HIP path "
                                  "(its weights are a download); start from pool / spatial activations")

    def read_statistics(self, npz_path, activations):
        obj = np.load(npz_path)
        if "mu" in list(obj.keys()):
            return FIDStatistics(obj["mu"], obj["sigma"]), FIDStatistics(obj["mu_s"], obj["sigma_s"])
        return tuple(self.compute_statistics(x) for x in activations)

    def compute_statistics(self, activations):
        return compute_statistics(activations)

    def compute_inception_score(self, activations, split_size=5000):
        if self.softmax_head is None:
            raise ValueError("Evaluator.compute_inception_score: no softmax_weight was given to the constructor")
        return compute_inception_score(activations, self.softmax_head, split_size, self.softmax_batch_size)

    def compute_prec_recall(self, activations_ref, activations_sample):
        return compute_prec_recall(activations_ref, activations_sample, self.manifold_estimator)

    def compute_kid(self, activations_ref, activations_sample, **kwargs):
        return compute_kid(activations_ref, activations_sample, **kwargs)

    def compute_density_coverage(self, activations_ref, activations_sample, nearest_k=5):
        return compute_density_coverage(activations_ref, activations_sample, nearest_k, self.manifold_estimator)


def metrics_from_activations(ref_acts, sample_acts, ref_stats=None, ref_stats_spatial=None, softmax_weight=None, split_size=5000,
                             kid=None, density_coverage=None):
    """What calculate_metrics does after compute_activations: ref_acts / sample_acts are (pool [N, 2048], spatial [N, 2023])
    tuples; reference statistics that are given are used instead of being recomputed.  Returns dict(fid, sfid, precision, recall),
    and with a softmax_weight also inception_score, of the sample pool activations.  kid=True or a dict of compute_kid keywords adds
    kid and kid_std, density_coverage=True (nearest_k = 5) or an integer nearest_k adds density and coverage, all of the pool
    activations."""
    for name, acts in (("ref_acts", ref_acts), ("sample_acts", sample_acts)):
        if not isinstance(acts, (tuple, list)) or len(acts) != 2:
            raise ValueError(f"metrics_from_activations: {name} must be a (pool, spatial) pair")
    what = "metrics_from_activations"
    shapes = [[_as_tensor(a, what) for a in acts] for acts in (ref_acts, sample_acts)]
    _same_width(what, shapes[0][0], shapes[1][0])
    _same_width(what, shapes[0][1], shapes[1][1])
    head = None
    if softmax_weight is not None:
        head = softmax_weight if isinstance(softmax_weight, _SoftmaxHead) else _SoftmaxHead(softmax_weight, what)
        if head.width != shapes[1][0].shape[1]:
            raise ValueError(f"{what}: pool activations are {shapes[1][0].shape[1]} wide, softmax_weight is [{head.width}, {head.classes}]")
        _split_size(what, split_size)
    if kid is not None:
        if kid is not True and not isinstance(kid, dict):
            raise ValueError(f"{what}: kid must be True or a dict of compute_kid keywords, got {type(kid).__name__}")
        kid = {} if kid is True else dict(kid)
        try:
            _kid_args(what, shapes[0][0], shapes[1][0], **kid)
        except TypeError as e:
            raise ValueError(f"{what}: kid holds a keyword compute_kid does not take ({e})") from None
    if density_coverage is not None:
        density_coverage = _dc_args(what, shapes[0][0], shapes[1][0], 5 if density_coverage is True else density_coverage)[2]
    ref_pool = _device_features(ref_acts[0], "metrics_from_activations")
    sample_pool = _device_features(sample_acts[0], "metrics_from_activations")
    ref_stats = ref_stats if ref_stats is not None else compute_statistics(ref_pool)
    ref_stats_spatial = ref_stats_spatial if ref_stats_spatial is not None else compute_statistics(ref_acts[1])
    sample_stats, sample_stats_spatial = compute_statistics(sample_pool), compute_statistics(sample_acts[1])
    prec, recall = compute_prec_recall(ref_pool, sample_pool)
    out = dict(fid=float(sample_stats.frechet_distance(ref_stats)), sfid=float(sample_stats_spatial.frechet_distance(ref_stats_spatial)),
               precision=prec, recall=recall)
    if head is not None:
        out["inception_score"] = compute_inception_score(sample_pool, head, split_size)
    if kid is not None:
        out["kid"], out["kid_std"] = compute_kid(ref_pool, sample_pool, **kid)
    if density_coverage is not None:
        out["density"], out["coverage"] = compute_density_coverage(ref_pool, sample_pool, density_coverage)
    return out

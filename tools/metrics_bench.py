#!/usr/bin/env python3
"""Times the evaluation metrics of vaw_amd.evaluator on synthetic activations.

    python tools/metrics_bench.py [--sizes 10000 50000] [--out FILE.json]
    python tools/metrics_bench.py --inception-score [--sizes 10000 50000] [--out FILE.json]
    python tools/metrics_bench.py --kid [--sizes 50000] [--out FILE.json]
    python tools/metrics_bench.py --density-coverage [--sizes 50000] [--out FILE.json]

Activations are non-negative and of low rank plus noise, like pooled ReLU features: max(z P + off + 0.01 noise, 0) with rank 64,
generated on the device from a seed; the sample set is drawn with z scaled by 0.8 and shifted by 0.5.  Per N it reports the median
over the repeats (after one warm-up of the same shapes) of
  * compute_prec_recall at D = 2048, device tensors in, two floats out (host clock around a call that ends in the read-back of the
    flags), and of its three pairwise launches alone (device events): two k-smallest launches and one within-radius launch, with the
    achieved f32 rate 2 N^2 D / t of each against the 157.3 TFLOP/s peak of the f32 matrix pipe;
  * compute_statistics at D = 2048 and D = 2023 (host clock, the [D, D] float64 read-back included) and of its covariance kernel
    alone (device events), with the f64 rate 2 N D^2 / t -- the FLOP of the full product, of which the kernel computes the upper
    triangle;
  * at N = 10000 only, the host baseline: the same arithmetic in numpy (float32 distances through the norm expansion in row blocks,
    np.partition / comparisons; float64 np.mean / np.cov).  The reference's TensorFlow path cannot run without TensorFlow.
With --inception-score it times the Inception score instead (D = 2048, C = 1008, the weight 3 / sqrt(D) randn as in the tests): the
head product vaw_head_logits alone (device events, rate 2 N D C / t), the float64 row pass, class sums and finish alone, and
compute_inception_score end to end (device activations in, one float out); at N = 10000 the host baseline is float32 numpy, the
arithmetic the reference's TensorFlow graph and its numpy tail perform.
With --kid it times the polynomial-kernel row sums (D = 2048, degree 3, gamma 1 / D, coef0 1): one launch of the full sets N x N, and
the KID protocol shape, 100 subsets of 1000 rows of the N-row sets through two index tables in one launch, each beside
vaw_pairwise_within at the same nu, nv, D (for the protocol shape one 1000 x 1000 launch, times the 100 subsets); then
polynomial_mmd2 and compute_kid end to end, and at the protocol shape the host baseline, float64 numpy on gathered copies (three
subsets, scaled to 100).  With --density-coverage it times vaw_pairwise_count_within N x N beside vaw_pairwise_within, and
compute_density_coverage end to end (nearest_k = 5).  vaw_pairwise_within is the same kernel, instruction for instruction, as the
one before the two entry points were added, so it stands for the parent commit.
One JSON object is printed (and written to --out).  It needs the GPU: there is no host path to time."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaw_amd  # noqa: E402
from vaw_amd import evaluator as ev, ops  # noqa: E402

PEAK_F32_TFLOPS = 157.3
RANK = 64


def features(n, d, seed, sample):
    g = torch.Generator(device="cuda").manual_seed(seed)
    proj = torch.randn(RANK, d, device="cuda", generator=g) / RANK ** 0.5
    off = torch.rand(d, device="cuda", generator=g) + 0.5
    g2 = torch.Generator(device="cuda").manual_seed(seed + 1 + int(sample))
    z = torch.randn(n, RANK, device="cuda", generator=g2)
    if sample:
        z = 0.8 * z + 0.5
    return torch.clamp_min(z @ proj + off + 0.01 * torch.randn(n, d, device="cuda", generator=g2), 0).contiguous()


def host_clock(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def device_clock(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return times


def summary(times):
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times), repeats=len(times))


def host_prec_recall(f1, f2, k=3, block=2000):
    """float32 numpy restatement of compute_prec_recall (distances through the norm expansion, row blocks of `block`)."""
    def dist(u, nu, v, nv):
        return np.maximum(nu[:, None] - 2 * (u @ v.T) + nv[None, :], 0)

    n1, n2 = (f1 * f1).sum(1), (f2 * f2).sum(1)

    def radii(f, n):
        out = np.empty(len(f), np.float32)
        for i in range(0, len(f), block):
            out[i:i + block] = np.partition(dist(f[i:i + block], n[i:i + block], f, n), k, axis=1)[:, k]
        return out

    r1, r2 = radii(f1, n1), radii(f2, n2)
    in1, in2 = np.zeros(len(f1), bool), np.zeros(len(f2), bool)
    for i in range(0, len(f1), block):
        d = dist(f1[i:i + block], n1[i:i + block], f2, n2)
        in1[i:i + block] = (d <= r2[None, :]).any(1)
        in2 |= (d <= r1[i:i + block, None]).any(0)
    return float(in2.mean()), float(in1.mean())


def host_inception_score(acts, w, split_size=5000):
    """float32 numpy: softmax(acts @ w), then the reference's expression per split."""
    logits = acts @ w
    e = np.exp(logits - logits.max(1, keepdims=True))
    preds = e / e.sum(1, keepdims=True)
    scores = []
    for i in range(0, len(preds), split_size):
        part = preds[i:i + split_size]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return float(np.mean(scores))


def inception_rows(args):
    d, c, split = 2048, 1008, 5000
    g = torch.Generator(device="cuda").manual_seed(100)
    w = torch.randn(d, c, device="cuda", generator=g) * 3 / d ** 0.5
    head = ev._SoftmaxHead(w)
    wt = head.class_major()
    sizes = {}
    for n in args.sizes:
        reps = args.repeats if n <= 20000 else max(3, args.repeats // 2 + 1)
        x = features(n, d, 0, True)
        row = dict(inception_score=ev.compute_inception_score(x, head, split))
        row["compute_inception_score"] = summary(host_clock(lambda: ev.compute_inception_score(x, head, split), 1, reps))
        logits = torch.empty(n, c, device="cuda", dtype=torch.float32)
        s = summary(device_clock(lambda: ops.head_logits(x, wt, logits), 1, reps))
        s["tflops_f32"] = 2.0 * n * d * c / s["median_s"] * 1e-12
        s["share_of_f32_peak"] = s["tflops_f32"] / PEAK_F32_TFLOPS
        row["head_logits"] = s
        lse, h = ops.is_rows(logits)
        colsum = torch.zeros(-(-n // split), c, device="cuda", dtype=torch.float64)
        row["is_rows"] = summary(device_clock(lambda: ops.is_rows(logits, False, lse, h), 1, reps))
        row["is_colsums"] = summary(device_clock(lambda: ops.is_colsums(logits, lse, 0, split, colsum), 1, reps))
        row["is_finish"] = summary(device_clock(lambda: ops.is_finish(h, colsum, split), 1, reps))
        if n == args.host_baseline_at:
            xh, wh = x.cpu().numpy(), w.cpu().numpy()
            host_inception_score(xh[:1000], wh)
            t0 = time.perf_counter()
            row["host_numpy_inception_score"] = host_inception_score(xh, wh, split)
            row["host_numpy_inception_score_s"] = time.perf_counter() - t0
            row["host_threads"] = torch.get_num_threads()
        sizes[str(n)] = row
        del x, logits
        torch.cuda.empty_cache()
    return sizes


def rated(times, flop):
    s = summary(times)
    s["tflops_f32"] = flop / s["median_s"] * 1e-12
    s["share_of_f32_peak"] = s["tflops_f32"] / PEAK_F32_TFLOPS
    return s


def within_launch(u, v):
    """One vaw_pairwise_within launch on u x v with one radius per point (the radii of the sets themselves)."""
    est = ev.ManifoldEstimator()
    nu, nv = ops.row_sqnorms(u), ops.row_sqnorms(v)
    ru, rv = torch.from_numpy(est.manifold_radii(u)).cuda(), torch.from_numpy(est.manifold_radii(v)).cuda()
    u_in = torch.zeros(len(u), 1, device="cuda", dtype=torch.uint8)
    v_in = torch.zeros(len(v), 1, device="cuda", dtype=torch.uint8)
    return lambda: ops.pairwise_within(u, v, nu, nv, ru, rv, u_in, v_in)


def host_kid_subset(x, y, gamma):
    """float64 numpy: the unbiased cubic-kernel MMD^2 of two gathered subsets."""
    m = len(x)
    kxx, kyy, kxy = ((gamma * (a @ b.T) + 1.0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
    return (kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2 * kxy.mean()


def kid_rows(args):
    d, subsets, size = 2048, 100, 1000
    gamma = 1.0 / d
    sizes = {}
    for n in args.sizes:
        reps = args.repeats if n <= 20000 else max(3, args.repeats // 2 + 1)
        ref, sample = features(n, d, 0, False), features(n, d, 0, True)
        row = dict(kid=ev.compute_kid(ref, sample), mmd2_full_sets=ev.polynomial_mmd2(ref, sample))
        row["polysum_full"] = rated(device_clock(lambda: ops.pairwise_polysum(ref, sample, gamma, 1.0, 3), 1, reps), 2.0 * n * n * d)
        row["within_full"] = rated(device_clock(within_launch(ref, sample), 1, reps), 2.0 * n * n * d)
        row["polysum_full_over_within"] = row["polysum_full"]["median_s"] / row["within_full"]["median_s"]
        ri, si = ev.kid_subset_indices(n, n, subsets, size, 0)
        ri, si = torch.from_numpy(ri).cuda(), torch.from_numpy(si).cuda()
        row["polysum_protocol"] = rated(device_clock(lambda: ops.pairwise_polysum(ref, sample, gamma, 1.0, 3, ri, si), 1, reps),
                                        2.0 * subsets * size * size * d)
        one = rated(device_clock(within_launch(ref[:size].contiguous(), sample[:size].contiguous()), 1, reps), 2.0 * size * size * d)
        row["within_one_subset"] = one
        row["polysum_protocol_over_100_within"] = row["polysum_protocol"]["median_s"] / (subsets * one["median_s"])
        row["compute_kid"] = summary(host_clock(lambda: ev.compute_kid(ref, sample), 1, reps))
        row["polynomial_mmd2"] = summary(host_clock(lambda: ev.polynomial_mmd2(ref, sample), 1, reps))
        if n == args.sizes[0]:
            xh, yh = ref.cpu().numpy(), sample.cpu().numpy()
            rj, sj = ri.cpu().numpy(), si.cpu().numpy()
            t0 = time.perf_counter()
            for b in range(3):
                host_kid_subset(xh[rj[b]].astype(np.float64), yh[sj[b]].astype(np.float64), gamma)
            row["host_numpy_kid_s_scaled_to_100_subsets"] = (time.perf_counter() - t0) * subsets / 3
            row["host_threads"] = torch.get_num_threads()
        sizes[str(n)] = row
        del ref, sample
        torch.cuda.empty_cache()
    return sizes


def density_coverage_rows(args):
    d = 2048
    sizes = {}
    for n in args.sizes:
        reps = args.repeats if n <= 20000 else max(3, args.repeats // 2 + 1)
        ref, sample = features(n, d, 0, False), features(n, d, 0, True)
        row = dict(density_coverage=ev.compute_density_coverage(ref, sample))
        row["compute_density_coverage"] = summary(host_clock(lambda: ev.compute_density_coverage(ref, sample), 1, reps))
        est = ev.ManifoldEstimator(nhood_sizes=(5,))
        radii = torch.from_numpy(est.manifold_radii(ref)).cuda()
        n_ref, n_sample = ops.row_sqnorms(ref), ops.row_sqnorms(sample)
        counts = torch.zeros(n, 1, device="cuda", dtype=torch.int32)
        covered = torch.zeros(n, 1, device="cuda", dtype=torch.uint8)
        row["count_within"] = rated(device_clock(lambda: ops.pairwise_count_within(sample, ref, n_sample, n_ref, radii, counts, covered), 1, reps),
                                    2.0 * n * n * d)
        row["within"] = rated(device_clock(within_launch(sample, ref), 1, reps), 2.0 * n * n * d)
        row["count_within_over_within"] = row["count_within"]["median_s"] / row["within"]["median_s"]
        sizes[str(n)] = row
        del ref, sample
        torch.cuda.empty_cache()
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-baseline-at", type=int, default=10000)
    ap.add_argument("--inception-score", action="store_true", help="time the Inception score instead of FID / precision / recall")
    ap.add_argument("--kid", action="store_true", help="time the polynomial-kernel row sums and KID instead")
    ap.add_argument("--density-coverage", action="store_true", help="time the counts under radii and density / coverage instead")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs the GPU: the metric kernels have no host path"
    vaw_amd.lib()
    result = dict(gpu=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), peak_f32_tflops=PEAK_F32_TFLOPS, sizes={})
    for n in ([] if args.inception_score or args.kid or args.density_coverage else args.sizes):
        reps = args.repeats if n <= 20000 else max(3, args.repeats // 2 + 1)
        row = {}
        ref, sample = features(n, 2048, 0, False), features(n, 2048, 0, True)
        est = ev.ManifoldEstimator()
        row["precision_recall"] = ev.compute_prec_recall(ref, sample)
        row["compute_prec_recall"] = summary(host_clock(lambda: ev.compute_prec_recall(ref, sample), 1, reps))
        n1, n2 = ops.row_sqnorms(ref), ops.row_sqnorms(sample)
        r1 = torch.from_numpy(est.manifold_radii(ref)).cuda()
        r2 = torch.from_numpy(est.manifold_radii(sample)).cuda()
        u_in = torch.zeros(n, 1, device="cuda", dtype=torch.uint8)
        v_in = torch.zeros(n, 1, device="cuda", dtype=torch.uint8)
        flop = 2.0 * n * n * 2048
        for name, fn in (("ksmallest_ref", lambda: ops.pairwise_ksmallest(ref, ref, 4, n1, n1)),
                         ("ksmallest_sample", lambda: ops.pairwise_ksmallest(sample, sample, 4, n2, n2)),
                         ("within", lambda: ops.pairwise_within(ref, sample, n1, n2, r1, r2, u_in, v_in))):
            s = summary(device_clock(fn, 1, reps))
            s["tflops_f32"] = flop / s["median_s"] * 1e-12
            s["share_of_f32_peak"] = s["tflops_f32"] / PEAK_F32_TFLOPS
            row[name] = s
        for d in (2048, 2023):
            x = ref if d == 2048 else features(n, d, 3, False)
            row[f"compute_statistics_d{d}"] = summary(host_clock(lambda: ev.compute_statistics(x), 1, reps))
            mu = ops.col_mean_f64(x)
            row[f"col_mean_f64_d{d}"] = summary(device_clock(lambda: ops.col_mean_f64(x), 1, reps))
            s = summary(device_clock(lambda: ops.cov_f64(x, mu), 1, reps))
            s["tflops_f64_full_product"] = 2.0 * n * d * d / s["median_s"] * 1e-12
            row[f"cov_f64_d{d}"] = s
            if n == args.host_baseline_at:
                xh = x.cpu().numpy()
                t0 = time.perf_counter()
                x64 = xh.astype(np.float64)
                x64.mean(0), np.cov(x64, rowvar=False)
                row[f"host_numpy_statistics_d{d}_s"] = time.perf_counter() - t0
        if n == args.host_baseline_at:
            f1, f2 = ref.cpu().numpy(), sample.cpu().numpy()
            t0 = time.perf_counter()
            row["host_numpy_precision_recall"] = host_prec_recall(f1, f2)
            row["host_numpy_prec_recall_s"] = time.perf_counter() - t0
            row["host_threads"] = torch.get_num_threads()
        result["sizes"][str(n)] = row
        del ref, sample
        torch.cuda.empty_cache()
    if args.inception_score:
        result["sizes"] = inception_rows(args)
    if args.kid:
        result["kid"] = kid_rows(args)
    if args.density_coverage:
        result["density_coverage"] = density_coverage_rows(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Likelihood evaluation timings (run on the GPU box).
    python tools/bpd_bench.py [--batch 32] [--T 1000] [--chunks 1,4,16] [--repeats 3] [--dtype bf16] [--skip-loop]

1. calc_bpd_loop on a learn_sigma DiT-B/4 (32 x 32 x 4 latents, LEARNED_RANGE, linear schedule): wall time of the whole loop
   (host clock around a device synchronise) per t_chunk, the configurations alternating inside every repeat.
2. vaw_bpd_terms alone against the unfused composition of existing pieces that yields the same three quantities
   (sample_step kind 0 + torch ops for the two MSEs + vb_terms), at the row count of the largest chunk, over rotating
   buffer sets larger than the 256 MiB Infinity Cache; device events.  Algorithmic bytes of the fused pass: 20 B/element."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaw_amd  # noqa: E402
from vaw_amd import ops  # noqa: E402


def diffusion(T, sched="linear"):
    args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=True, p2_gamma=1, p2_k=1, time_dist=["uniform"], cpu_rng=False)
    return vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule(sched, T),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.LEARNED_RANGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=(T != 1000))


def bench_loop(a, d):
    torch.manual_seed(0)
    model = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=1000, learn_sigma=True,
                          compute_dtype=a.dtype).to("cuda").eval()
    with torch.no_grad():
        for p in model.parameters():          # the zero-initialised output layers would make every timestep trivial
            if p.requires_grad:
                p.add_(torch.randn_like(p) * 0.02)
    if hasattr(model, "mark_weights_changed"):
        model.mark_weights_changed()
    x0 = torch.randn(a.batch, 4, 32, 32, device="cuda").clamp(-1, 1)
    kw = {"y": torch.randint(0, 1000, (a.batch,), device="cuda")}
    chunks = [int(c) for c in a.chunks.split(",")]
    warm = diffusion(max(chunks) * 2, "cosine")                           # every stacked batch size once, outside the timed window
    for K in chunks:
        warm.calc_bpd_loop(model, x0, model_kwargs=kw, t_chunk=K)
    torch.cuda.synchronize()
    times, totals = {K: [] for K in chunks}, {}
    for _ in range(a.repeats):
        for K in chunks:
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = d.calc_bpd_loop(model, x0, model_kwargs=kw, t_chunk=K)
            torch.cuda.synchronize()
            times[K].append(time.perf_counter() - t0)
            totals[K] = out["total_bpd"]
    for K in chunks:
        ts = sorted(times[K])
        dev = float((totals[K] - totals[chunks[0]]).abs().max() / totals[chunks[0]].abs().max())
        print(f"calc_bpd_loop DiT-B/4 {a.dtype} batch {a.batch} T {d.num_timesteps} t_chunk {K:3d}: median {ts[len(ts) // 2]:7.3f} s  "
              f"min {ts[0]:7.3f}  max {ts[-1]:7.3f}  ({1e3 * ts[len(ts) // 2] / d.num_timesteps:6.3f} ms/timestep)  "
              f"total_bpd vs t_chunk {chunks[0]}: {dev:.2e}", flush=True)


def timeit(fns, iters):
    for f in fns:
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def bench_kernel(a, d):
    rows = a.batch * max(int(c) for c in a.chunks.split(","))
    n = 4 * 32 * 32
    nset = max(2, int(400e6 // (rows * n * 4 * 5)) + 1)
    t = torch.randint(0, d.num_timesteps, (rows,), device="cuda")
    coef = d._sample_rows(t)
    ra, rm1 = coef[:, 6].view(-1, 1, 1, 1), coef[:, 7].view(-1, 1, 1, 1)
    sets = []
    for _ in range(nset):
        out2 = torch.randn(rows, 8, 32, 32, device="cuda")
        out2[:, 4:].clamp_(-1, 1)
        m, v = torch.split(out2, 4, dim=1)
        x0, nz = torch.randn(rows, 4, 32, 32, device="cuda").clamp(-1, 1), torch.randn(rows, 4, 32, 32, device="cuda")
        sets.append((m, v, x0, d.q_sample(x0, t, nz), nz))
    res = tuple(torch.empty(rows, 1, device="cuda") for _ in range(3))

    def fused(s):
        return lambda: ops.bpd_terms(s[0], s[1], s[2], s[3], s[4], coef, 0, 2, False, out=res, col=0, group=rows)

    def unfused(s):
        def run():
            m, v, x0, xt, nz = s
            pred = ops.sample_step(0, m, v, xt, None, coef, 0, 2, False)["pred_xstart"]
            xm = ((pred - x0) ** 2).flatten(1).mean(1)
            ms = (((ra * xt - pred) / rm1 - nz) ** 2).flatten(1).mean(1)
            return ops.vb_terms(m, v, x0, xt, coef, 0, 2), xm, ms
        return run

    f_us = timeit([fused(s) for s in sets], a.iters)
    u_us = timeit([unfused(s) for s in sets], a.iters)
    nbytes = 20.0 * rows * n
    print(f"vaw_bpd_terms  rows {rows} x {n}: {f_us:8.1f} us  {nbytes / 1e6:7.1f} MB algorithmic  {nbytes / f_us / 1e6:5.2f} TB/s", flush=True)
    print(f"unfused composition (sample_step + torch + vb_terms): {u_us:8.1f} us  -> fused is {u_us / f_us:4.1f}x faster", flush=True)
    got, ref = fused(sets[0])(), unfused(sets[0])()
    for nm, g, r in zip(("vb", "xstart_mse", "mse"), got, ref):
        print(f"  {nm}: max|fused - unfused| / max|unfused| = {float((g.flatten() - r).abs().max() / r.abs().max()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--chunks", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bpd_bench.py measures on the GPU only")
    d = diffusion(a.T)
    bench_kernel(a, d)
    if not a.skip_loop:
        bench_loop(a, d)


if __name__ == "__main__":
    main()

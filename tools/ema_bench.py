#!/usr/bin/env python3
"""What tracking power-function EMA profiles (post-hoc EMA, vaw_amd.PowerEMA) costs at the parameter count of DiT-XL/2.

    python tools/ema_bench.py [--workload dit_xl2] [--reps 30] [--rounds 5] [--steps 10] [--warmup 5] [--no-step] [--time-limit 540]

Kernels: vaw_ema_profiles_update for K = 1, 2, 4 over buffers of the model's flat size, and adamw_ema_kernel (FusedAdamW's pass
with the EMA folded in and the bf16 shadow written) over the same count in the same process; HIP events around --reps back-to-back
launches after 5 warm-up launches, Python call included.  Bytes are those the algorithm needs: (4 + 8 K) per parameter for the
profiles, 38 per parameter for AdamW + EMA + shadow (p, g, m, v, ema read; p, m, v, ema written; 2 B of shadow).  The buffers are
far larger than any cache, so every launch streams from HBM.
Step: a Trainer step (bf16, FusedAdamW, deferred loss read-out: the step of bench.py) without and with args.ema_sigma_rels =
(0.05, 0.10); each arm has a Trainer of its own and they take turns in one process, host clock around --steps steps ending in a
device synchronise, median over --rounds rounds with the smallest and largest beside it.  One JSON line per figure."""
import argparse
import json
import os
import signal
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps, warm=5):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps          # ms


def kernels(n, reps):
    import torch

    from vaw_amd import ops
    dev = "cuda"
    p = torch.randn(n, device=dev)
    out = {}
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for K in (1, 2, 4):
        bufs = [torch.zeros(n, device=dev) for _ in range(K)]
        gamma = torch.tensor([16.97, 6.94, 3.56, 1.0][:K], dtype=torch.float64, device=dev)
        coef = torch.zeros(K, dtype=torch.float64, device=dev)
        for _ in range(3):
            ops.ema_profiles_coef(step, gamma, coef)          # c_t < 1: the arithmetic path of every later step
        ms = timed(lambda: ops.ema_profiles_update(p, bufs, coef), reps)
        nbytes = (4 + 8 * K) * n
        out[f"profiles_K{K}"] = dict(kernel="ema_profiles_update", K=K, n=n, ms=round(ms, 4), bytes=nbytes, TBps=round(nbytes / ms / 1e9, 3))
        print(json.dumps(out[f"profiles_K{K}"]), flush=True)
        del bufs
    coef_ms = timed(lambda: ops.ema_profiles_coef(step, gamma, coef), 200)
    print(json.dumps(dict(kernel="ema_profiles_coef", K=4, us=round(1e3 * coef_ms, 2))), flush=True)
    g, m, v, e = (torch.randn(n, device=dev) * 1e-3 for _ in range(4))
    v.abs_()
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
    ms = timed(lambda: ops.adamw_ema_step(p, g, m, v, e, shadow, 1e-4, 0.9, 0.95, 1e-8, 0.0, 10, 0.9999, None, 0.0, False), reps)
    nbytes = 38 * n
    out["adamw_ema"] = dict(kernel="adamw_ema", n=n, ms=round(ms, 4), bytes=nbytes, TBps=round(nbytes / ms / 1e9, 3))
    print(json.dumps(out["adamw_ema"]), flush=True)
    ref = out["adamw_ema"]["TBps"]
    print(json.dumps(dict(summary="B/s of the profile update over B/s of adamw_ema in this run",
                          **{k: round(r["TBps"] / ref, 3) for k, r in out.items() if k != "adamw_ema"})), flush=True)


def make_arm(wl_name, rels):
    import torch

    import bench
    import vaw_amd
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[wl_name]
    args = bench.make_args(**({"ema_sigma_rels": rels} if rels else {}))
    model, ema_model = bench.build(vaw_amd, wl, args, dev, 0)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    return vaw_amd.Trainer(args, dev, model, ema_model, opt, sched, diff, bench._Loader(bench.synth_batches(wl["batch"], 3, dev, 3)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="dit_xl2")
    ap.add_argument("--reps", type=int, default=30, help="back-to-back launches per kernel figure")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="optimizer steps of an arm per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--time-limit", type=int, default=540, help="seconds for the whole run")
    a = ap.parse_args()
    signal.alarm(a.time_limit)                     # default action: the process ends

    import torch
    if not torch.cuda.is_available():
        print("ema_bench: needs the GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    import bench
    import vaw_amd
    probe = bench.make_model(vaw_amd, bench.WORKLOADS[a.workload])          # on the host: only its flat size is wanted
    probe.ensure_flat()
    n = probe._flat.numel()
    del probe
    print(json.dumps(dict(workload=a.workload, flat_elements=n)), flush=True)
    kernels(n, a.reps)
    torch.cuda.empty_cache()
    if a.no_step:
        return 0
    names = {"K0": None, "K2": (0.05, 0.10)}
    arms = {k: make_arm(a.workload, r) for k, r in names.items()}
    count = {k: 0 for k in arms}

    def run(k, steps):
        for _ in range(steps):
            count[k] += 1
            arms[k].train_step(count[k])
    for k in arms:
        run(k, a.warmup)
    per_round = {k: [] for k in arms}
    order = list(arms)
    for r in range(a.rounds):
        for k in (order if r % 2 == 0 else order[::-1]):          # alternate the order: no arm always follows the other
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k, a.steps)
            torch.cuda.synchronize()
            per_round[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
    med = {}
    for k in arms:
        v = sorted(per_round[k])
        med[k] = v[len(v) // 2]
        print(json.dumps(dict(arm=k, workload=a.workload, step_ms=round(med[k], 3), step_ms_min=round(v[0], 3), step_ms_max=round(v[-1], 3),
                              rounds=a.rounds, steps_per_round=a.steps)), flush=True)
    print(json.dumps(dict(summary=f"{a.workload}: Trainer step with two tracked profiles over the step without",
                          K2_over_K0_ms=round(med["K2"] - med["K0"], 3), ratio=round(med["K2"] / med["K0"], 4))), flush=True)
    signal.alarm(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())

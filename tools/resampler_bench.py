#!/usr/bin/env python3
"""What loss-aware timestep sampling costs a training step: no sampler, the host "loss-second-moment" sampler and the
device-resident "loss-second-moment-device" sampler on the same model, batch and data.

    python tools/resampler_bench.py [--batches 256,32] [--rounds 7] [--steps 20] [--warmup 10] [--graph] [--time-limit 540]

Per batch size every arm gets a Trainer of its own (DiT-B/4, bf16, FusedAdamW, deferred loss read-out: the headline step of
bench.py) and the arms take turns inside ONE process: a round runs --steps optimizer steps of each arm, the host clock around
them ends in a device synchronise (a launch returns before its kernel finishes, and the host sampler's cost IS host time), and
the figure of an arm is the median over --rounds rounds of the per-step time, with the smallest and largest round beside it --
the spread is the noise a difference has to exceed.  Both samplers start from the same full history, so p is not uniform.
--graph adds the no-sampler and device-sampler arms with the step captured into a hipGraph (the host sampler refuses that).
Then the two kernels alone: HIP events around 200 back-to-back launches each.  One JSON line per arm and per kernel, then a
summary line per batch size.  --time-limit ends the whole run (SIGALRM) if it is still going after that many seconds."""
import argparse
import json
import os
import signal
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_arm(name, batch, hist):
    import torch

    import bench
    import vaw_amd
    from vaw_amd import resample
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["dit_b4"]
    sampler = {"none": None, "host": "loss-second-moment", "device": "loss-second-moment-device"}[name.split("+")[0]]
    args = bench.make_args(hip_graph=name.endswith("+graph"), schedule_sampler=sampler)
    model, ema_model = bench.build(vaw_amd, wl, args, dev, 0)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, dev, model, ema_model, opt, sched, diff, bench._Loader(bench.synth_batches(batch, 4, dev, 3)))
    if sampler == "loss-second-moment":
        tr.schedule_sampler = resample.host_from_state_dict(diff, hist)
    elif sampler:
        tr.schedule_sampler.load_state_dict(hist)
    return tr


def kernel_times(batch, hist, reps=200):
    """microseconds per launch of the draw and the update kernel at this batch size, T = 1000, H = 10, full history"""
    from types import SimpleNamespace

    import torch

    import vaw_amd
    s = vaw_amd.DeviceLossSecondMomentResampler(SimpleNamespace(num_timesteps=hist["ring"].shape[0]), "cuda", hist["ring"].shape[1])
    s.load_state_dict(hist)
    u = torch.rand(batch, dtype=torch.float64, device="cuda")
    loss = torch.rand(batch, device="cuda")
    t, _ = s._draw(u)
    out = {}
    for what, fn in (("draw", lambda: s._draw(u)), ("update", lambda: s.update_with_all_losses(t, loss))):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out[what] = round(1e3 * e0.elapsed_time(e1) / reps, 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="256,32", help="the headline batch and the 32-image strong-scaling shard")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="optimizer steps of an arm per round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graph", action="store_true", help="also time the no-sampler and device-sampler arms with args.hip_graph=True")
    ap.add_argument("--time-limit", type=int, default=540, help="seconds for the whole run")
    a = ap.parse_args()
    signal.alarm(a.time_limit)                     # default action: the process ends

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("resampler_bench: needs the GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    rng = np.random.RandomState(0)
    hist = {"ring": torch.from_numpy(10.0 ** rng.uniform(-2, 0.5, size=(1000, 10))), "seen": torch.full((1000,), 10, dtype=torch.int64)}
    names = ["none", "host", "device"] + (["none+graph", "device+graph"] if a.graph else [])
    for batch in (int(b) for b in a.batches.split(",")):
        arms = {n: make_arm(n, batch, hist) for n in names}
        step = {n: 0 for n in names}

        def run(n, k):
            for _ in range(k):
                step[n] += 1
                arms[n].train_step(step[n])
        for n in names:
            run(n, a.warmup)
        torch.cuda.synchronize()
        per_round = {n: [] for n in names}
        for r in range(a.rounds):
            for n in (names if r % 2 == 0 else names[::-1]):          # alternate the order: no arm always follows the same one
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(n, a.steps)
                torch.cuda.synchronize()
                per_round[n].append(1e3 * (time.perf_counter() - t0) / a.steps)
        res = {}
        for n in names:
            v = sorted(per_round[n])
            res[n] = dict(arm=n, batch=batch, step_ms=round(v[len(v) // 2], 4), step_ms_min=round(v[0], 4), step_ms_max=round(v[-1], 4),
                          rounds=a.rounds, steps_per_round=a.steps, graph_taken=arms[n]._graph is not None)
            print(json.dumps(res[n]), flush=True)
        k = kernel_times(batch, hist)
        print(json.dumps(dict(kernels_us=k, batch=batch, T=1000, H=10)), flush=True)
        base = res["none"]["step_ms"]
        print(json.dumps(dict(summary=f"DiT-B/4 bf16 batch {batch}", **{f"{n}_ms": res[n]["step_ms"] for n in names},
                              host_over_none_us=round(1e3 * (res["host"]["step_ms"] - base), 1),
                              device_over_none_us=round(1e3 * (res["device"]["step_ms"] - base), 1),
                              none_spread_us=round(1e3 * (res["none"]["step_ms_max"] - res["none"]["step_ms_min"]), 1),
                              draw_us=k["draw"], update_us=k["update"])), flush=True)
        del arms
        torch.cuda.empty_cache()
    signal.alarm(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())

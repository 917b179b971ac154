#!/usr/bin/env python3
"""What the step guard (vaw_amd.StepGuard, FusedAdamW.attach_guard) costs at the trainable-parameter counts of DiT-B/4 and DiT-XL/2.

    python tools/guard_bench.py [--workloads dit_b4,dit_xl2] [--reps 20] [--rounds 7] [--time-limit 540]

Four arms over the same buffers of a model's trainable size, in one process, taking turns round by round (the order reversed every
other round, so no arm always follows the same one); HIP events around --reps back-to-back launches of an arm, Python call
included, after every arm has been warmed on those shapes:
  adamw          vaw_adamw_ema_step: AdamW + EMA + bf16 shadow, the pass every step runs today
  guarded_ok1    vaw_adamw_ema_step_guarded with ok = 1: the same pass behind the verdict
  guarded_ok0    vaw_adamw_ema_step_guarded with ok = 0: a refused step (reads the verdict, moves nothing)
  check          vaw_sumsq + vaw_step_guard: the verdict itself (a run that clips has the sum of squares already)
Bytes are those the shapes imply: 38 per parameter for the pass (p, g, m, v, ema read; p, m, v, ema written; 2 B of shadow), 4 per
parameter for the check (g read), none for a refused step.  The buffers are far larger than any cache.  One JSON line per arm and
workload: the median over the rounds with the smallest and largest beside it, and GB/s from the median."""
import argparse
import json
import os
import signal
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps          # ms


def measure(name, n, reps, rounds):
    import torch

    import vaw_amd
    from vaw_amd import ops
    dev = "cuda"
    p = torch.randn(n, device=dev)
    g, m, v, e = (torch.randn(n, device=dev) * 1e-3 for _ in range(4))
    v.abs_()
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
    sumsq = torch.zeros(1, device=dev)
    guard = vaw_amd.StepGuard(dev)
    one, zero = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def adamw(ok=None):
        kw = {} if ok is None else {"ok": ok}
        ops.adamw_ema_step(p, g, m, v, e, shadow, 1e-4, 0.9, 0.95, 1e-8, 0.0, 10, 0.9999, None, 0.0, False, **kw)

    def check():
        ops.sumsq(g, sumsq)
        guard.check(sumsq)

    arms = {"adamw": (adamw, 38 * n), "guarded_ok1": (lambda: adamw(one), 38 * n), "guarded_ok0": (lambda: adamw(zero), 0),
            "check": (check, 4 * n)}
    for fn, _ in arms.values():
        for _ in range(5):
            fn()
    ms = {k: [] for k in arms}
    order = list(arms)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(timed(arms[k][0], reps))
    out = {}
    for k, (_, nbytes) in arms.items():
        s = sorted(ms[k])
        med = s[len(s) // 2]
        out[k] = dict(workload=name, arm=k, n=n, ms=round(med, 4), ms_min=round(s[0], 4), ms_max=round(s[-1], 4), bytes=nbytes,
                      GBps=round(nbytes / med / 1e6, 1), rounds=rounds, reps=reps)
        print(json.dumps(out[k]), flush=True)
    c = guard.counters()
    assert c["skipped_nonfinite"] == 0 and c["applied"] == c["steps"], c          # the timed gradient was finite throughout
    base = out["adamw"]["ms"]
    print(json.dumps(dict(summary=f"{name}: over the unguarded pass of this run", guarded_ok1=round(out["guarded_ok1"]["ms"] / base, 4),
                          guarded_ok0=round(out["guarded_ok0"]["ms"] / base, 4), check=round(out["check"]["ms"] / base, 4),
                          guard_on=round((out["guarded_ok1"]["ms"] + out["check"]["ms"]) / base, 4))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="dit_b4,dit_xl2")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches of an arm per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--time-limit", type=int, default=540, help="seconds for the whole run")
    a = ap.parse_args()
    signal.alarm(a.time_limit)                     # default action: the process ends

    import torch
    if not torch.cuda.is_available():
        print("guard_bench: needs the GPU (a CPU run measures nothing)", file=sys.stderr)
        return 1
    import bench
    import vaw_amd
    for name in a.workloads.split(","):
        probe = bench.make_model(vaw_amd, bench.WORKLOADS[name])          # on the host: only its trainable size is wanted
        probe.ensure_flat()
        n = probe._flat_n_train
        del probe
        measure(name, n, a.reps, a.rounds)
        torch.cuda.empty_cache()
    signal.alarm(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())

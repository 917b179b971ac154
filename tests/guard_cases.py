"""What tests/test_guard_cpu.py and tests/test_gpu_guard.py share: the decision rule of vaw_step_guard restated in numpy float64, and
the hand-written sequence of sums of squares both run it on.  Nothing here imports the package."""
import numpy as np

COUNTERS = ("ok", "steps", "applied", "skipped_nonfinite", "skipped_spike", "in_a_row")
STATS = ("last_norm", "mean", "max_norm")
NEW_ENTRY_POINTS = ("vaw_step_guard", "vaw_adamw_ema_step_guarded", "vaw_adamw_ema_step_guarded_dev", "vaw_fp8_scale_update_finite",
                    "vaw_resampler_update_finite")

# spike test: factor 3 over a mean of decay 0.9, live once 3 steps were applied
SPIKE = dict(spike_factor=3.0, spike_beta=0.9, spike_warmup=3)
# (sum of squares as the kernel reads it, the verdict a reader works out by hand, why)
SEQUENCE = [
    (4.0, 1, "norm 2: the first applied step sets the mean"),
    (9.0, 1, "norm 3: mean 2.1"),
    (100.0, 1, "norm 10 > 3 * 2.1, but only 2 steps were applied: before the warm-up nothing is a spike; mean 2.89"),
    (float("inf"), 0, "overflowed sum"),
    (float("nan"), 0, "NaN gradient"),
    (6.25, 1, "norm 2.5 after two refusals: applied, the streak ends; mean 2.851"),
    (1.0e4, 0, "norm 100 > 3 * 2.851 with 4 steps applied: a spike"),
    (2.25, 1, "norm 1.5: recovery"),
    (0.0, 1, "an all-zero gradient is finite"),
    (3.0e38, 0, "finite in f32, norm 1.7e19: a spike, not an overflow"),
    (1.0, 1, "norm 1: recovery again"),
]


def guard_reference(sumsqs, spike_factor=None, spike_beta=0.99, spike_warmup=100):
    """The state after every launch of vaw_step_guard over `sumsqs`, from a zero state: [(counters dict, stats dict)].  float64,
    one rounding per operation; the factor and the sum of squares are the f32 values the launch receives."""
    c, s = dict.fromkeys(COUNTERS, 0), dict.fromkeys(STATS, 0.0)
    factor, beta, out = np.float64(np.float32(spike_factor or 0.0)), np.float64(spike_beta), []
    for ss in sumsqs:
        ss = np.float32(ss)
        with np.errstate(invalid="ignore"):
            norm = np.sqrt(np.float64(ss))
        finite = bool(np.isfinite(ss))
        spike = finite and factor > 0 and c["applied"] >= spike_warmup and bool(norm > factor * np.float64(s["mean"]))
        ok = finite and not spike
        if ok:
            s["mean"] = float(norm) if c["applied"] == 0 else float(beta * np.float64(s["mean"]) + (np.float64(1.0) - beta) * norm)
            s["max_norm"] = float(max(np.float64(s["max_norm"]), norm))
            c["applied"] += 1
            c["in_a_row"] = 0
        else:
            c["skipped_spike" if finite else "skipped_nonfinite"] += 1
            c["in_a_row"] += 1
        c["steps"] += 1
        c["ok"] = int(ok)
        s["last_norm"] = float(norm)
        out.append((dict(c), dict(s)))
    return out

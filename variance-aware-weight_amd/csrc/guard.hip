// Step guard (vaw_amd/guard.py: StepGuard; optim.py: FusedAdamW.attach_guard): the verdict on one optimizer step, formed on the
// device from the step's sum of squared gradients (vaw_sumsq, the scalar the global-norm clip already needs) and left in device
// memory for vaw_adamw_ema_step_guarded to branch on.  No host value enters the launch, so it sits in a captured step like any other.
//
// One thread: the state is six int32 and four f64, every word has one writer, plain vector stores, no atomics.  IEEE f64 with every
// operation rounded on its own (the Makefile's EXTRA_guard and the pragma below), so the numpy restatement in tests/guard_cases.py
// reproduces the statistics.
#include "common.h"

#pragma clang fp contract(off)

// counters: {ok, steps, applied, skipped_nonfinite, skipped_spike, in_a_row};  stats: {last_norm, mean, max_norm, 0}
__global__ void __launch_bounds__(64) step_guard_kernel(const float* __restrict__ sumsq, int32_t* __restrict__ counters,
                                                        double* __restrict__ stats, float spike_factor, double spike_beta,
                                                        int spike_warmup) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float ss = sumsq[0];
    const double norm = sqrt((double)ss);
    const bool finite = (__float_as_int(ss) & 0x7f800000) != 0x7f800000;
    const int32_t applied = counters[2];
    const double mean = stats[1];
    const bool spike = finite && spike_factor > 0.f && applied >= spike_warmup && norm > (double)spike_factor * mean;
    const bool ok = finite && !spike;
    if (ok) {
        stats[1] = applied == 0 ? norm : spike_beta * mean + (1.0 - spike_beta) * norm;
        const double mx = stats[2];
        stats[2] = norm > mx ? norm : mx;
        counters[2] = applied + 1;
        counters[5] = 0;
    } else {
        const int which = finite ? 4 : 3;
        counters[which] = counters[which] + 1;
        counters[5] = counters[5] + 1;
    }
    counters[1] = counters[1] + 1;
    stats[0] = norm;
    counters[0] = ok ? 1 : 0;
}

extern "C" int vaw_step_guard(const float* sumsq, int32_t* counters, double* stats, float spike_factor, double spike_beta,
                              int spike_warmup, vaw_stream stream) {
    VAW_CHECK_ARG(sumsq && counters && stats, "step_guard: sumsq / counters / stats is NULL");
    VAW_CHECK_ARG(((uintptr_t)sumsq & 3) == 0 && ((uintptr_t)counters & 3) == 0 && ((uintptr_t)stats & 7) == 0,
                  "step_guard: sumsq and counters 4-byte aligned, stats 8-byte aligned");
    VAW_CHECK_ARG(!(spike_factor > 0.f) || spike_factor > 1.f, "step_guard: spike_factor %g must be more than 1 (or <= 0: no spike test)",
                  (double)spike_factor);
    VAW_CHECK_ARG(spike_beta >= 0.0 && spike_beta < 1.0 && spike_warmup >= 0, "step_guard: spike_beta %g must be in [0, 1), spike_warmup %d not negative",
                  spike_beta, spike_warmup);
    step_guard_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sumsq, counters, stats, spike_factor, spike_beta, spike_warmup);
    VAW_CHECK_LAUNCH("step_guard");
    return VAW_OK;
}

"""Step guard: the device refuses an optimizer step whose gradient is not finite, or whose norm spikes above its running mean.

A step of this engine can be one replayed hipGraph with the loss left on the device: no host code sees a value of it, so only the
device can refuse an update.  `StepGuard` owns the verdict's state -- six int32 counters and four f64 statistics in device memory
(include/vaw_hip.h: vaw_step_guard) -- and `FusedAdamW.attach_guard(guard)` puts two things into the step: one one-thread launch
that turns the step's sum of squared gradients (the scalar the global-norm clip already forms) into the verdict, and the guarded
form of the fused AdamW + EMA pass, which leaves the masters, both moments, the EMA and the bf16 shadow untouched when the verdict
is "no".  Nothing here synchronises with the host except `counters()` and `stats()`, which say so.

Not `torch.amp.GradScaler`: there is no loss scale to back off (bf16 and the fp8 path's per-tensor scales keep the f32 exponent range),
and a skipped step still counts as a step -- the Adam step count behind the bias corrections and the LR schedule advance, because
both stay host arithmetic that must not depend on a device value.  GradScaler skips `optimizer.step()` on the host and the
scheduler's step is then the caller's to skip; here a run with the guard attached and nothing skipped is bitwise the run without it,
and a skipped step costs one step of schedule.
"""
import torch

from . import _lib as L

COUNTERS = ("ok", "steps", "applied", "skipped_nonfinite", "skipped_spike", "in_a_row")
STATS = ("last_norm", "mean", "max_norm")


class StepGuard:
    """spike_factor None: only non-finite gradients are refused.  spike_factor F > 1: after `spike_warmup` applied steps, a step
    whose gradient norm exceeds F times the running mean of the applied steps' norms (decay `spike_beta`) is refused too.
    GPU only: the verdict is formed and read on the device."""

    def __init__(self, device, spike_factor=None, spike_beta=0.99, spike_warmup=100):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.VawError(f"StepGuard keeps its verdict on the GPU: got device '{device}' (no CPU fallback exists by design)")
        if spike_factor is not None and not float(spike_factor) > 1.0:
            raise ValueError(f"StepGuard: spike_factor {spike_factor!r} must be more than 1 (None: no spike test)")
        if not 0.0 <= float(spike_beta) < 1.0:
            raise ValueError(f"StepGuard: spike_beta {spike_beta!r} must be in [0, 1)")
        if int(spike_warmup) != spike_warmup or int(spike_warmup) < 0:
            raise ValueError(f"StepGuard: spike_warmup {spike_warmup!r} must be a non-negative integer")
        self.device = device
        self.spike_factor = None if spike_factor is None else float(spike_factor)
        self.spike_beta, self.spike_warmup = float(spike_beta), int(spike_warmup)
        # allocated once, written in place ever after: a captured step keeps the addresses
        self._counters = torch.zeros(L.GUARD_COUNTERS, dtype=torch.int32, device=device)
        self._stats = torch.zeros(L.GUARD_STATS, dtype=torch.float64, device=device)
        self.device = self._counters.device          # ("cuda" -> "cuda:<current>")

    @property
    def ok(self):
        """device int32 [1]: the last verdict, the word the guarded update branches on"""
        return self._counters[0:1]

    def check(self, sumsq):
        """Enqueue the verdict on `sumsq` (device f32 [1], the step's sum of squared gradients).  Never synchronises."""
        L.need_cuda(sumsq)
        L.check(L.lib().vaw_step_guard(L.ptr(sumsq), L.ptr(self._counters), L.ptr(self._stats), self.spike_factor or 0.0,
                                       self.spike_beta, self.spike_warmup, L.stream_ptr()), "vaw_step_guard")

    def counters(self):
        """{ok, steps, applied, skipped_nonfinite, skipped_spike, in_a_row} as host ints.  Synchronises: for inspection and the
        trainer's periodic check, not for the step."""
        return dict(zip(COUNTERS, (int(x) for x in self._counters.cpu().tolist())))

    def stats(self):
        """{last_norm, mean, max_norm} of the gradient norm as host floats.  Synchronises."""
        return dict(zip(STATS, (float(x) for x in self._stats.cpu().tolist())))

    def state_dict(self):
        return {"counters": self._counters.detach().cpu().clone(), "stats": self._stats.detach().cpu().clone(),
                "spike_factor": self.spike_factor, "spike_beta": self.spike_beta, "spike_warmup": self.spike_warmup}

    def load_state_dict(self, sd):
        counters, stats = torch.as_tensor(sd["counters"]), torch.as_tensor(sd["stats"])
        if tuple(counters.shape) != tuple(self._counters.shape) or tuple(stats.shape) != tuple(self._stats.shape):
            raise L.VawError(f"load_state_dict: guard state {tuple(counters.shape)} / {tuple(stats.shape)} does not fit "
                             f"{tuple(self._counters.shape)} / {tuple(self._stats.shape)}")
        self._counters.copy_(counters.to(torch.int32))          # in place: a captured step keeps the addresses
        self._stats.copy_(stats.to(torch.float64))

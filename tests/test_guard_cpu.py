"""CPU-only checks of the step guard (vaw_amd.StepGuard, FusedAdamW.attach_guard, Trainer's args.skip_nonfinite): the C ABI binds
the five new entry points as the header declares them, the host classes refuse what they must before anything is launched, and the
float64 restatement of the decision rule that the GPU tests hold the kernel to (tests/guard_cases.py) agrees with a sequence worked
out by hand.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, base_args

import abi_cases
import guard_cases as gc
import vaw_amd


def test_new_entry_points_are_bound_as_declared():
    lib = vaw_amd.lib()
    for name in gc.NEW_ENTRY_POINTS:
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name), name
        abi_cases.assert_bound_as_declared(lib, name)
    # the guarded entries are today's with one more argument, the verdict, in front of the stream
    sig = abi_cases.signatures()
    for plain, guarded in (("vaw_adamw_ema_step", "vaw_adamw_ema_step_guarded"), ("vaw_adamw_ema_step_dev", "vaw_adamw_ema_step_guarded_dev")):
        assert sig[guarded][0] is sig[plain][0] and sig[guarded][1][:-2] == sig[plain][1][:-1] and sig[guarded][1][-1] == sig[plain][1][-1]
    for plain, finite in (("vaw_fp8_scale_update", "vaw_fp8_scale_update_finite"), ("vaw_resampler_update", "vaw_resampler_update_finite")):
        assert sig[finite] == sig[plain]
    assert (vaw_amd._lib.GUARD_COUNTERS, vaw_amd._lib.GUARD_STATS) == (len(gc.COUNTERS), len(gc.STATS) + 1)
    mk = open(os.path.join(REPO, "variance-aware-weight_amd", "csrc", "Makefile")).read()
    assert "guard.hip" in mk and re.search(r"EXTRA_guard\s*=\s*-ffp-contract=off", mk)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    assert lib.vaw_step_guard(None, None, None, 0.0, 0.99, 100, None) == -1                       # NULL buffers
    assert "NULL" in lib.vaw_last_error_string().decode()
    assert lib.vaw_step_guard(4, 8, 16, 1.0, 0.99, 100, None) == -1                               # a factor of 1 refuses every step
    assert lib.vaw_step_guard(4, 8, 16, 3.0, 1.0, 100, None) == -1                                # beta = 1: the mean never moves
    assert lib.vaw_step_guard(4, 8, 16, 3.0, 0.5, -1, None) == -1
    assert lib.vaw_step_guard(4, 8, 12, 3.0, 0.5, 1, None) == -1                                  # stats not 8-byte aligned
    args = [16, 16, 16, 16, 0, 0, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 0.1, 0.1, 0.0, 0, 0.0, 0]
    assert lib.vaw_adamw_ema_step_guarded(*args, None, None) == -1                                # no verdict
    assert "ok" in lib.vaw_last_error_string().decode()
    assert lib.vaw_adamw_ema_step_guarded(*args[:6], 0, *args[7:], 4, None) == -1                 # n = 0
    assert lib.vaw_fp8_scale_update_finite(None, 4, None) == -1
    assert lib.vaw_resampler_update_finite(None, None, 4, 7, 0, None, None, None, None) == -1


def test_step_guard_refuses_a_cpu_device_and_bad_arguments():
    with pytest.raises(vaw_amd.VawError, match="GPU"):
        vaw_amd.StepGuard("cpu")
    with pytest.raises(vaw_amd.VawError, match="GPU"):
        vaw_amd.StepGuard(torch.device("cpu"), spike_factor=3.0)
    # (the arguments are checked before a byte is allocated: this runs without a GPU)
    for bad in (1.0, 0.5, 0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="spike_factor"):
            vaw_amd.StepGuard("cuda", spike_factor=bad)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="spike_beta"):
            vaw_amd.StepGuard("cuda", spike_factor=3.0, spike_beta=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="spike_warmup"):
            vaw_amd.StepGuard("cuda", spike_factor=3.0, spike_warmup=bad)


@pytest.mark.parametrize("extra", [dict(skip_nonfinite=True), dict(skip_grad_spike=4.0)])
def test_trainer_refuses_the_guard_with_a_torch_optimizer(extra):
    model = torch.nn.Linear(4, 4)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="FusedAdamW"):
        vaw_amd.Trainer(base_args(**extra), torch.device("cpu"), model, None, opt, None, None, [])
    # absent or off: the constructor goes on as it always did
    for off in (dict(), dict(skip_nonfinite=False, skip_grad_spike=None)):
        tr = vaw_amd.Trainer(base_args(**off), torch.device("cpu"), model, None, opt, None, None, [])
        assert tr.guard is None


def test_attach_guard_wants_a_step_guard():
    assert vaw_amd.FusedAdamW.attach_guard.__doc__ and "torch.amp" in vaw_amd.guard.__doc__
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=1, num_heads=2, num_classes=10)
    opt = vaw_amd.FusedAdamW(m, lr=1e-3)
    assert opt.guard is None
    with pytest.raises(TypeError, match="StepGuard"):
        opt.attach_guard(object())
    opt.attach_guard(None)
    assert opt.guard is None


def test_restatement_agrees_with_the_sequence_worked_out_by_hand():
    seq = gc.SEQUENCE
    kinds = [np.isfinite(np.float32(s)) for s, _, _ in seq]
    assert any(np.isinf(np.float32(s)) for s, _, _ in seq) and any(np.isnan(np.float32(s)) for s, _, _ in seq) and sum(kinds) >= 5
    states = gc.guard_reference([s for s, _, _ in seq], **gc.SPIKE)
    assert [c["ok"] for c, _ in states] == [v for _, v, _ in seq], [(c["ok"], why) for (c, _), (_, _, why) in zip(states, seq)]
    # the spike before the warm-up was applied, the one after it refused
    assert states[2][0]["applied"] == 3 and states[2][0]["skipped_spike"] == 0 and states[6][0]["skipped_spike"] == 1
    # means worked out by hand (the module's comments), to the rounding of a few float64 operations
    for i, mean in ((0, 2.0), (1, 2.1), (2, 2.89), (5, 2.851), (7, 2.7159), (8, 2.44431)):
        assert states[i][1]["mean"] == pytest.approx(mean, rel=1e-12), i
    # a refusal moves neither the mean nor the maximum nor `applied`; the streak counts and ends
    for i in (3, 4, 6, 9):
        assert states[i][1]["mean"] == states[i - 1][1]["mean"] and states[i][1]["max_norm"] == states[i - 1][1]["max_norm"]
        assert states[i][0]["applied"] == states[i - 1][0]["applied"]
    assert [c["in_a_row"] for c, _ in states] == [0, 0, 0, 1, 2, 0, 1, 0, 0, 1, 0]
    assert np.isinf(states[3][1]["last_norm"]) and np.isnan(states[4][1]["last_norm"]) and states[9][1]["last_norm"] > 1e19
    last_c, last_s = states[-1]
    assert last_c == dict(ok=1, steps=11, applied=7, skipped_nonfinite=2, skipped_spike=2, in_a_row=0)
    assert last_s["max_norm"] == 10.0 and last_s["last_norm"] == 1.0
    for c, _ in states:
        assert c["steps"] == c["applied"] + c["skipped_nonfinite"] + c["skipped_spike"]
    # without a factor only the non-finite sums are refused
    plain = gc.guard_reference([s for s, _, _ in seq])
    assert [c["ok"] for c, _ in plain] == [int(k) for k in kinds] and plain[-1][0]["skipped_spike"] == 0

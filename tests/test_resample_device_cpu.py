"""CPU-only checks of the device-resident timestep sampler ("loss-second-moment-device"): the C ABI declares and exports its two
entry points, the registry builds it and refuses a CPU device, the host names ignore `device=`, the history moves between the
host and the device format without a kernel, and checkpoints written before the sampler key existed still load.  No kernel is
launched here (the entry points' argument checks run before any launch)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO

import vaw_amd
from vaw_amd import resample


def _diff(T=7, **args):
    return SimpleNamespace(num_timesteps=T, args=SimpleNamespace(**args))


def test_header_declares_and_library_exports_both_entry_points():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    lib = vaw_amd.lib()
    for name in ("vaw_resampler_update", "vaw_resampler_draw"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
    assert int(re.search(r"#define\s+VAW_RESAMPLER_MAX_T\s+(\d+)", hdr).group(1)) == vaw_amd._lib.RESAMPLER_MAX_T
    src = open(os.path.join(REPO, "variance-aware-weight_amd", "csrc", "Makefile")).read()
    assert "resample.hip" in src and re.search(r"EXTRA_resample\s*=\s*-ffp-contract=off", src)


def test_entry_points_refuse_bad_sizes_before_any_launch():
    """T just over what the draw's one workgroup holds, and non-positive sizes: VAW_ERR_INVALID with a message, nothing enqueued
    (the checks come before the pointers are looked at, so this runs without a GPU)."""
    lib = vaw_amd.lib()
    T = vaw_amd._lib.RESAMPLER_MAX_T + 1
    assert lib.vaw_resampler_draw(None, None, T, 10, 0.001, None, 0, None, None, None, None) == -1
    msg = lib.vaw_last_error_string().decode()
    assert str(T) in msg and str(T - 1) in msg
    assert lib.vaw_resampler_draw(None, None, 0, 10, 0.001, None, 0, None, None, None, None) == -1
    assert lib.vaw_resampler_draw(None, None, 7, 3, 1.5, None, 0, None, None, None, None) == -1
    assert lib.vaw_resampler_draw(None, None, 7, 3, 0.001, None, 0, None, None, None, None) == -1       # NULL history
    assert lib.vaw_resampler_update(None, None, 4, 7, 0, None, None, None, None) == -1
    assert lib.vaw_resampler_update(None, None, -1, 7, 3, None, None, None, None) == -1
    assert lib.vaw_resampler_update(None, None, 4, 7, 3, None, None, None, None) == -1                  # NULL history
    with pytest.raises(vaw_amd.VawError, match="resampler_update"):
        vaw_amd._lib.check(-1, "vaw_resampler_update")


def test_registry_names():
    d = _diff(7)
    assert isinstance(resample.create_named_schedule_sampler("uniform", d, device="cpu"), vaw_amd.UniformSampler)
    assert isinstance(resample.create_named_schedule_sampler("uniform", d, device="cuda"), vaw_amd.UniformSampler)
    for dev in (None, "cpu", "cuda", torch.device("cpu")):
        h = resample.create_named_schedule_sampler("loss-second-moment", d, device=dev)
        assert type(h) is vaw_amd.LossSecondMomentResampler and h._ring.shape == (7, 10)
    assert type(resample.create_named_schedule_sampler("loss-second-moment", d)) is vaw_amd.LossSecondMomentResampler
    with pytest.raises(NotImplementedError):
        resample.create_named_schedule_sampler("loss-third-moment", d, device="cuda")
    with pytest.raises(NotImplementedError):
        resample.create_named_schedule_sampler("nope", d)
    assert vaw_amd.DeviceLossSecondMomentResampler is resample.DeviceLossSecondMomentResampler


@pytest.mark.parametrize("dev", ["cpu", torch.device("cpu")])
def test_cpu_device_raises(dev):
    with pytest.raises(vaw_amd.VawError, match="GPU"):
        resample.create_named_schedule_sampler("loss-second-moment-device", _diff(7), device=dev)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.DeviceLossSecondMomentResampler(_diff(7), dev)
    host = vaw_amd.LossSecondMomentResampler(_diff(7), 3)
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.DeviceLossSecondMomentResampler.from_host(host, dev)


def test_trainer_refuses_the_device_sampler_on_a_cpu_device_and_keeps_the_host_refusal():
    from conftest import base_args
    d = _diff(7)
    mk = lambda **kw: vaw_amd.Trainer(base_args(**kw), torch.device("cpu"), torch.nn.Linear(2, 2), None,
                                      torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), None, d, [])
    with pytest.raises(vaw_amd.VawError):
        mk(schedule_sampler="loss-second-moment-device")
    with pytest.raises(ValueError, match="hip_graph"):
        mk(schedule_sampler="loss-second-moment", hip_graph=True)
    tr = mk(schedule_sampler="loss-second-moment")
    assert type(tr.schedule_sampler) is vaw_amd.LossSecondMomentResampler and not tr._device_sampler


def test_history_round_trips_between_host_and_device_format():
    """from_host / to_host go through these two helpers; the state itself needs no kernel."""
    rng = np.random.RandomState(3)
    host = vaw_amd.LossSecondMomentResampler(_diff(7), history_per_term=3, uniform_prob=0.01)
    for _ in range(9):
        host.update_with_all_losses(rng.randint(0, 7, 5).tolist(), rng.rand(5).astype(np.float32).tolist())
    sd = resample.host_state_dict(host)
    assert sd["ring"].dtype == torch.float64 and sd["seen"].dtype == torch.int64
    assert sd["ring"].shape == (7, 3) and sd["seen"].shape == (7,)
    before = host._ring.copy()
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd["ring"].zero_()               # the state is a copy: writing to it does not reach the host sampler
    np.testing.assert_array_equal(host._ring, before)
    back = resample.host_from_state_dict(host.diffusion, sd2, 3, 0.01)
    np.testing.assert_array_equal(back._ring, host._ring)
    np.testing.assert_array_equal(back._seen, host._seen)
    assert back._ring.dtype == np.float64 and back._seen.dtype == np.int64
    assert back.history_per_term == 3 and back.uniform_prob == 0.01
    np.testing.assert_array_equal(back.weights(), host.weights())
    # and they continue identically
    for s in (back, host):
        s.update_with_all_losses([6, 6, 0], [0.5, 0.25, 2.0])
    np.testing.assert_array_equal(back._ring, host._ring)
    np.testing.assert_array_equal(back._seen, host._seen)
    with pytest.raises(ValueError):
        resample.host_from_state_dict(_diff(8), sd2, 3, 0.01)


class _FakeSampler:
    def __init__(self):
        self.sd = {"ring": torch.arange(6, dtype=torch.float64).reshape(3, 2), "seen": torch.tensor([2, 5, 9])}
        self.loaded = None

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd):
        self.loaded = sd


def test_checkpoint_carries_the_sampler_state_and_old_files_load(tmp_path):
    args = SimpleNamespace(logdir=str(tmp_path), model="m", mean_type="EPSILON", path_type="cosine")
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    # a file from before the key existed: loads, and the sampler is left alone
    old = vaw_amd.save_checkpoint(args, 1, model, opt)
    assert "schedule_sampler" not in torch.load(old, weights_only=True)
    s = _FakeSampler()
    ck = vaw_amd.load_checkpoint(old, model=model, optimizer=opt, schedule_sampler=s)
    assert s.loaded is None and ck["step"] == 1
    # a host sampler has no state_dict: nothing is written for it
    host = vaw_amd.LossSecondMomentResampler(_diff(7))
    p2 = vaw_amd.save_checkpoint(args, 2, model, opt, schedule_sampler=host)
    assert "schedule_sampler" not in torch.load(p2, weights_only=True)
    vaw_amd.load_checkpoint(p2, model=model, schedule_sampler=host)
    # with a state_dict: written under the new key and handed back on load
    p3 = vaw_amd.save_checkpoint(args, 3, model, opt, schedule_sampler=s)
    raw = torch.load(p3, weights_only=True)
    assert set(raw["schedule_sampler"]) == {"ring", "seen"}
    vaw_amd.load_checkpoint(p3, model=model, optimizer=opt, schedule_sampler=s)
    assert torch.equal(s.loaded["ring"], s.sd["ring"]) and torch.equal(s.loaded["seen"], s.sd["seen"])
    assert s.loaded["ring"].dtype == torch.float64 and s.loaded["seen"].dtype == torch.int64
    # the old call forms are unchanged
    vaw_amd.load_checkpoint(p3, model, opt)

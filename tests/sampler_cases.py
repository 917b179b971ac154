"""Shared by test_sampler_cpu.py and test_gpu_sampler.py: how tests/golden/make_sampler_goldens.py set the reference's
Sampler up for each case of tests/golden/sampler.pt, restated for the package's classes."""
import torch

import vaw_amd
from conftest import SAMPLING_CASES, base_args, sampling_model, sampling_model_2c

BAND_REL = 1e-4


class Standin(torch.nn.Module):
    """The stand-in denoiser as a module (Sampler calls .eval() on its model)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, t, **kw):
        return self.fn(x, t, **kw)


def sampler_args(kind, st, **kw):
    a = dict(in_chans=3, class_cond=True, parallel=False, class_labels=None, amp=False, vae="ema", cpu_rng=True,
             guidance_scale=st["guidance_scale"], interval=tuple(st.get("interval", (-1.0, -1.0))),
             model_mode="flow" if kind == "flow" else "diffusion", solver=st.get("solver", "ddim"),
             sample_steps=st.get("sample_steps", 0), discretization="edm", schedule="linear", scaling="none",
             path_type=st.get("path_type", "cosine"), mean_type=st.get("mean_type", "EPSILON"), sampler_type="sde")
    a.update(kw)
    return base_args(**a)


def spaced(case, args):
    """SpacedDiffusion of a conftest.SAMPLING_CASES entry (its schedule, mean / variance type and respacing) + its stand-in."""
    _, sched, mt, vt, respacing, _, _, _ = next(c for c in SAMPLING_CASES if c[0] == case)
    learned = vt.startswith("LEARNED")
    args.learn_sigma = learned
    d = vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(1000, respacing), args=args,
                                betas=vaw_amd.get_named_beta_schedule(sched, 1000), model_mean_type=vaw_amd.ModelMeanType[mt],
                                model_var_type=vaw_amd.ModelVarType[vt], loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    return d, Standin(sampling_model_2c if learned else sampling_model)


def build(kind, st, args):
    if kind == "ddim":
        return spaced(st["case"], args)
    if kind == "flow":
        return vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType[st["mean_type"]]), Standin(sampling_model)
    return None, Standin(sampling_model)


def in_band(floats):
    """[B, H, W, C] mask of the bytes whose fixture value (x + 1) * 127.5 lies within 127.5 * (1e-4 + 1e-4 |x|) of an integer."""
    x = floats.double().permute(0, 2, 3, 1)
    v = (x + 1) * 127.5
    return (v - v.round()).abs() <= 127.5 * (BAND_REL + BAND_REL * x.abs())

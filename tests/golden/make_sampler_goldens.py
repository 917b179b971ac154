#!/usr/bin/env python3
"""Generate tests/golden/sampler.pt by running the UNMODIFIED reference's `Sampler.sample` (tools/sampler.py:97-269) on
CPU, driven with the stand-in denoisers of make_goldens.py under the CPU RNG stream.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_sampler_goldens.py

Only data is written: settings, the uint8 NHWC batches and label batches `sample` returns, and the float samples it hands to
`_inverse_normalize`.  Two conditions are asserted on the reference's own data (a case that breaks one wants another seed):
every stored float is finite and at most 1e4 in magnitude, and at most 15 % of a case's bytes have a pre-quantisation value
(x + 1) * 127.5 within 127.5 * (1e-4 + 1e-4 |x|) of an integer -- the band inside which a float difference at the test's
tolerance may move a byte by one level (about 5 % is expected from evenly spread fractional parts, plus pixels clipped to +-1)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import base_args, install_stubs, sampling_model, sampling_model_2c  # noqa: E402

SAMPLE_SIZE, IMAGE_SIZE, NUM_CLASSES, NUM_SAMPLES = 3, 8, 10, 6          # two batches of three 8 x 8 images
BAND_REL, BAND_MAX_SHARE = 1e-4, 0.15

# name, seed, kind, settings.  DDIM rows name an entry of conftest.SAMPLING_CASES (its schedule, mean / variance type and
# respacing; the reference's Sampler always runs eta = 0 with clipping).
#
# "saturating": read as an EPSILON model under guidance 2.5 the stand-in denoiser drives 50-62 % of the final pixels onto the
# clip at exactly +-1 (byte 0 / 255, an integer pre-quantisation value) whatever the seed, the schedule or the respacing --
# measured on all four EPSILON entries of SAMPLING_CASES with seeds 123 and 1 -- and the only LEARNED_RANGE entries are
# EPSILON ones.  The 15 % condition as stated cannot hold for them; it is asserted there on the bytes that are NOT exactly
# clipped, and both shares are stored and printed.  The fixed-variance entry is a START_X one, which meets it as stated.
CASES = [
    ("p20_x0_large/always", 123, "ddim", dict(case="p20_x0_large", guidance_scale=2.5, interval=(-1.0, -1.0))),
    ("p20_x0_large/interval", 123, "ddim", dict(case="p20_x0_large", guidance_scale=2.5, interval=(200.0, 700.0))),
    ("ddim10_eps_range_eta/always", 123, "ddim", dict(case="ddim10_eps_range_eta", guidance_scale=2.5, interval=(-1.0, -1.0), saturating=True)),
    ("ddim10_eps_range_eta/interval", 123, "ddim", dict(case="ddim10_eps_range_eta", guidance_scale=2.5, interval=(200.0, 700.0), saturating=True)),
    ("edm_heun", 123, "edm", dict(solver="heun", sample_steps=9, path_type="cosine", mean_type="VELOCITY", guidance_scale=2.5)),
    ("edm_euler", 123, "edm", dict(solver="euler", sample_steps=12, path_type="linear", mean_type="VELOCITY", guidance_scale=2.5)),
    ("flow_sde_heun", 123, "flow", dict(solver="heun", sample_steps=9, path_type="linear", mean_type="VELOCITY", guidance_scale=2.5)),
]
DDIM_CASES = {  # the two rows of conftest.SAMPLING_CASES used above: schedule, mean type, var type, respacing
    "p20_x0_large": ("cosine", "START_X", "FIXED_LARGE", "20"),
    "ddim10_eps_range_eta": ("linear", "EPSILON", "LEARNED_RANGE", "10"),
}


class Standin(torch.nn.Module):
    """The stand-in denoiser as a module (the Sampler calls .eval() on its model)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, t, **kw):
        return self.fn(x, t, **kw)


def sampler_args(kind, st):
    return base_args(in_chans=3, class_cond=True, parallel=False, class_labels=None, amp=False, vae="ema", cpu_rng=True,
                     guidance_scale=st["guidance_scale"], interval=tuple(st.get("interval", (-1.0, -1.0))),
                     model_mode="flow" if kind == "flow" else "diffusion", solver=st.get("solver", "ddim"),
                     sample_steps=st.get("sample_steps", 0), discretization="edm", schedule="linear", scaling="none",
                     path_type=st.get("path_type", "cosine"), mean_type=st.get("mean_type", "EPSILON"), sampler_type="sde")


def build(gd, R, kind, st, args):
    """(diffusion object, stand-in model) of a case, from the reference's modules (or the package's: same names)."""
    if kind == "ddim":
        sched, mt, vt, respacing = DDIM_CASES[st["case"]]
        learned = vt.startswith("LEARNED")
        args.learn_sigma = learned
        d = R.SpacedDiffusion(use_timesteps=R.space_timesteps(1000, respacing), args=args, betas=gd.get_named_beta_schedule(sched, 1000),
                              model_mean_type=gd.ModelMeanType[mt], model_var_type=gd.ModelVarType[vt], loss_type=gd.LossType.MSE,
                              rescale_timesteps=True, device="cpu")
        return d, Standin(sampling_model_2c if learned else sampling_model)
    if kind == "flow":
        return gd.FlowMatching(args=args, model_mean_type=gd.ModelMeanType[st["mean_type"]], device="cpu"), Standin(sampling_model)
    return None, Standin(sampling_model)          # EDM: the Sampler builds its own Net over the model


def band_share(floats, images):
    """(share of bytes whose pre-quantisation value lies in the boundary band, share that does so without being clipped)."""
    x = torch.cat([f.double().permute(0, 2, 3, 1).reshape(-1) for f in floats])
    v = (x + 1) * 127.5
    near = (v - v.round()).abs() <= 127.5 * (BAND_REL + BAND_REL * x.abs())
    assert x.numel() == sum(i.numel() for i in images)
    return float(near.double().mean()), float((near & (x.abs() != 1)).double().mean())


def main():
    install_stubs()
    torch.set_num_threads(8)
    from tools import gaussian_diffusion as gd
    from tools import respace as R
    from tools.sampler import Sampler
    out = {"sample_size": SAMPLE_SIZE, "image_size": IMAGE_SIZE, "num_classes": NUM_CLASSES, "num_samples": NUM_SAMPLES, "cases": {}}
    for name, seed, kind, st in CASES:
        args = sampler_args(kind, st)
        diffusion, model = build(gd, R, kind, st, args)
        s = Sampler(args, "cpu", model, diffusion)
        floats, finish = [], s._inverse_normalize
        s._inverse_normalize = lambda x: (floats.append(x.detach().clone()), finish(x))[1]
        torch.manual_seed(seed)
        images, labels = s.sample(NUM_SAMPLES, SAMPLE_SIZE, IMAGE_SIZE, NUM_CLASSES)
        images, labels = [torch.from_numpy(i) for i in images], [torch.from_numpy(l) for l in labels]
        assert len(images) == len(labels) == len(floats) == 2 and all(i.dtype == torch.uint8 and i.shape == (3, 8, 8, 3) for i in images)
        for f in floats:
            assert bool(torch.isfinite(f).all()) and float(f.abs().max()) <= 1e4, f"{name}: floats not finite / bounded"
        share, share_unclipped = band_share(floats, images)
        held = share_unclipped if st.get("saturating") else share
        assert held <= BAND_MAX_SHARE, f"{name}: {held:.3f} of the bytes lie in the boundary band (> {BAND_MAX_SHARE}): pick another seed"
        out["cases"][name] = {"kind": kind, "seed": seed, "settings": {k: (list(v) if isinstance(v, tuple) else v) for k, v in st.items()},
                              "images": images, "labels": labels, "floats": floats, "band_share": share,
                              "band_share_unclipped": share_unclipped}
        print(f"  {name}: labels {[l.tolist() for l in labels]} float dtype {floats[0].dtype} max|x| "
              f"{max(float(f.abs().max()) for f in floats):.4g} band share {share:.3f} (not clipped: {share_unclipped:.3f})", flush=True)
    path = os.path.join(HERE, "sampler.pt")
    torch.save(out, path)
    print("wrote sampler.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

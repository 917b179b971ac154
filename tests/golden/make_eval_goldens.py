#!/usr/bin/env python3
"""Generate tests/golden/eval_bpd.pt by running the UNMODIFIED reference's likelihood-evaluation side on CPU:
`calc_bpd_loop`, `_prior_bpd`, `q_mean_variance`, `q_posterior_mean_variance` and the `ddim_reverse_sample` walk
t = 0 .. T-1, driven with the stand-in denoisers of make_goldens.py under the CPU RNG stream.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_eval_goldens.py

Only data is written (inputs, settings, expected outputs).  Every stored array must be finite and bounded by 1e4 in
magnitude -- asserted below -- so that an ill-conditioned case cannot set the scale of an absolute tolerance."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import base_args, install_stubs, sampling_model, sampling_model_2c  # noqa: E402

# name, schedule, base T, mean type, var type, respacing (None = plain GaussianDiffusion), rescale_timesteps, clip_denoised
BPD_CASES = [
    ("lin_eps_range_50", "linear", 1000, "EPSILON", "LEARNED_RANGE", "50", True, True),
    ("cos_x0_large_20", "cosine", 1000, "START_X", "FIXED_LARGE", "20", True, True),
    ("lin_xprev_small_25", "linear", 1000, "PREVIOUS_X", "FIXED_SMALL", "25", True, True),
    ("lin_eps_range_1000", "linear", 1000, "EPSILON", "LEARNED_RANGE", "1000", True, True),
    ("lin_x0_learned_15_noclip", "linear", 1000, "START_X", "LEARNED", "15", True, False),
    ("plain_lin_x0_small_100", "linear", 100, "START_X", "FIXED_SMALL", None, False, True),
]
# The inversion walk is a chained map: with the stand-in denoiser read as START_X it expands (|x| grows from 1 to ~70 on
# the linear schedule, ~110 on cosine), and PREVIOUS_X without clipping leaves the 1e4 bound, so those are not pinned as
# trajectories (the kernel's START_X / PREVIOUS_X arithmetic is tested per step against float64 instead).
INV_CASES = [
    ("inv_lin_eps_range_50", "linear", 1000, "EPSILON", "LEARNED_RANGE", "50", True, True),
    ("inv_lin_eps_small_20_noclip", "linear", 1000, "EPSILON", "FIXED_SMALL", "20", True, False),
    ("inv_lin_xprev_large_25", "linear", 1000, "PREVIOUS_X", "FIXED_LARGE", "25", True, True),
    ("inv_plain_lin_eps_large_100", "linear", 100, "EPSILON", "FIXED_LARGE", None, False, True),
]


def check(name, tree):
    if isinstance(tree, dict):
        for k, v in tree.items():
            check(f"{name}/{k}", v)
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            check(f"{name}/{i}", v)
    elif isinstance(tree, torch.Tensor) and tree.is_floating_point():
        assert bool(torch.isfinite(tree).all()), f"{name}: not finite"
        assert float(tree.abs().max()) <= 1e4, f"{name}: max|value| = {float(tree.abs().max()):.3g} > 1e4"


def make(gd, R, sched, T, mt, vt, respacing, rescale):
    learned = vt.startswith("LEARNED")
    kw = dict(args=base_args(learn_sigma=learned, amp=False), betas=gd.get_named_beta_schedule(sched, T),
              model_mean_type=gd.ModelMeanType[mt], model_var_type=gd.ModelVarType[vt], loss_type=gd.LossType.MSE,
              rescale_timesteps=rescale, device="cpu")
    d = gd.GaussianDiffusion(**kw) if respacing is None else R.SpacedDiffusion(use_timesteps=R.space_timesteps(T, respacing), **kw)
    return d, (sampling_model_2c if learned else sampling_model)


def main():
    install_stubs()
    torch.set_num_threads(8)
    from tools import gaussian_diffusion as gd
    from tools import respace as R
    x0 = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(7)).clamp(-1, 1)
    y = torch.tensor([1, 5, 9])
    q_noise = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(11))
    out = {"x0": x0, "y": y, "q_noise": q_noise, "bpd": {}, "inv": {}}
    for name, sched, T, mt, vt, respacing, rescale, clip in BPD_CASES:
        d, model = make(gd, R, sched, T, mt, vt, respacing, rescale)
        n = d.num_timesteps
        torch.manual_seed(123)
        rec = {k: v.clone() for k, v in d.calc_bpd_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}).items()}
        rec["prior_only"] = d._prior_bpd(x0).clone()
        ts = [torch.tensor([0, n // 2, n - 1]), torch.tensor([n - 1, 1, n // 3])]
        rec["q_t"] = ts
        rec["q_mean_variance"] = [[v.clone() for v in d.q_mean_variance(x0, t)] for t in ts]
        rec["q_x_t"] = [d.q_sample(x0, t, noise=q_noise).clone() for t in ts]
        rec["q_posterior_mean_variance"] = [[v.clone() for v in d.q_posterior_mean_variance(x0, xt, t)]
                                            for t, xt in zip(ts, rec["q_x_t"])]
        rec["eps_from_xstart"] = [d._predict_eps_from_xstart(xt, t, x0).clone() for t, xt in zip(ts, rec["q_x_t"])]
        rec["n"] = n
        check(name, rec)
        out["bpd"][name] = rec
        print(f"  bpd {name}: T={n} total_bpd={rec['total_bpd'].tolist()} max|mse|={float(rec['mse'].abs().max()):.4g} "
              f"max|xstart_mse|={float(rec['xstart_mse'].abs().max()):.4g}", flush=True)
    for name, sched, T, mt, vt, respacing, rescale, clip in INV_CASES:
        d, model = make(gd, R, sched, T, mt, vt, respacing, rescale)
        n = d.num_timesteps
        torch.manual_seed(123)
        x, traj, preds = x0, [], []
        with torch.no_grad():
            for i in range(n):
                o = d.ddim_reverse_sample(model, x, torch.full((3,), i, dtype=torch.long), clip_denoised=clip, model_kwargs={"y": y})
                x = o["sample"]
                traj.append(x.clone())
                preds.append(o["pred_xstart"].clone())
        rec = {"first": traj[0], "mid": traj[n // 2], "final": traj[-1], "pred_first": preds[0], "pred_final": preds[-1], "n": n}
        check(name, rec)
        out["inv"][name] = rec
        print(f"  inv {name}: T={n} final std={float(traj[-1].std()):.4g} max|x|={float(traj[-1].abs().max()):.4g}", flush=True)
    torch.save(out, os.path.join(HERE, "eval_bpd.pt"))
    print("wrote eval_bpd.pt", os.path.getsize(os.path.join(HERE, "eval_bpd.pt")), "bytes")


if __name__ == "__main__":
    main()

"""Model- and step-level parity of the HIP DiT path with the reference (through golden fixtures) and with the
CPU oracle, plus size-independent properties at the BASELINE batch.  Run on the MI355X box: pytest -m gpu."""
import copy
import random

import numpy as np
import pytest
import torch

import model_grad_cases as grad_cases
from conftest import (Pbar, assert_fingerprints, base_args, load_json, load_pt, perturb_, synth_loader)

pytestmark = pytest.mark.gpu

import vaw_amd
from oracle import diffusion as od
from oracle import dit as odit
from oracle import trainer as otr

DEV = "cuda"


def _tiny(tag, g, dtype):
    torch.manual_seed(11)
    m = vaw_amd.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype=dtype,
                    **g[f"{tag}/kw"])
    return m


@pytest.mark.parametrize("tag", ["p2", "p4"])
def test_dit_tiny_fp32_matches_reference_golden(tag):
    g = load_pt("dit_tiny.pt")
    m = _tiny(tag, g, "fp32")
    assert_fingerprints(m.state_dict(), g[f"{tag}/init_sd"], 1e-6, 1e-9, "same seed => the reference's initial weights")
    m = m.to(DEV).train()
    x, t, y, gout = (g[f"{tag}/{k}"].to(DEV) for k in ("x", "t", "y", "gout"))
    out0, aux = m(x, t, y)
    assert aux is None and float(out0.abs().max()) == 0.0          # adaLN-Zero: exact zeros at init
    perturb_(m, 99)                                                   # same CPU generator stream as the fixture
    assert_fingerprints({k: v.cpu() for k, v in m.state_dict().items()}, g[f"{tag}/sd"], 1e-6, 1e-9, "perturbed")
    xr = x.clone().requires_grad_(True)
    out, _ = m(xr, t, y)
    (out * gout).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), g[f"{tag}/out"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(xr.grad.cpu(), g[f"{tag}/gx"], rtol=1e-4, atol=2e-5)
    grads = {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}
    assert_fingerprints(grads, g[f"{tag}/grads"], 1e-4, 2e-5, "parameter gradients")
    # gradient accumulation: a second backward adds (torch convention), zero_grad_flat resets
    g1 = {k: v.clone() for k, v in grads.items()}
    out, _ = m(xr, t, y)
    (out * gout).sum().backward()
    for k, p in m.named_parameters():
        if p.grad is not None:
            torch.testing.assert_close(p.grad.cpu(), 2 * g1[k], rtol=1e-5, atol=1e-6)
    m.zero_grad_flat()
    out, _ = m(xr, t, y)
    (out * gout).sum().backward()
    for k, p in m.named_parameters():
        if p.grad is not None:
            torch.testing.assert_close(p.grad.cpu(), g1[k], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("tag", ["p2", "p4"])
def test_dit_tiny_bf16_close_to_reference(tag):
    """Throughput mode (bf16 operands, f32 accumulate).  Tolerance 3e-2 of each tensor's rms: bf16 has 8
    significant bits and activations pass through ~10 roundings."""
    g = load_pt("dit_tiny.pt")
    m = _tiny(tag, g, "bf16").to(DEV).train()
    perturb_(m, 99)
    x, t, y, gout = (g[f"{tag}/{k}"].to(DEV) for k in ("x", "t", "y", "gout"))
    xr = x.clone().requires_grad_(True)
    out, _ = m(xr, t, y)
    (out * gout).sum().backward()
    ref = g[f"{tag}/out"]
    assert float((out.detach().cpu() - ref).norm() / ref.norm()) < 3e-2
    assert float((xr.grad.cpu() - g[f"{tag}/gx"]).norm() / g[f"{tag}/gx"].norm()) < 5e-2
    for k, p in m.named_parameters():
        if p.grad is not None:
            gl2 = float(g[f"{tag}/grads"][k]["stats"][2])
            assert abs(float(p.grad.double().norm()) - gl2) <= 5e-2 * gl2 + 1e-4, k
    # a norm does not see a swapped, permuted, transposed or sign-flipped gradient: whole tensors against the float64 oracle at the
    # same weights and inputs, each within twice the oracle's own bf16-autocast distance (tests/model_grad_cases.py)
    om = odit.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, **g[f"{tag}/kw"])
    om.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    g64, e_ref = grad_cases.oracle_yardstick("dit", om.train(), *(g[f"{tag}/{k}"] for k in ("x", "t", "y", "gout")))
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    got.update({grad_cases.OUT: out.detach(), grad_cases.GX: xr.grad})
    worst, n = grad_cases.hold_whole_tensors(got, g64, e_ref)
    assert n == len(g64)
    print(f"\ndit_tiny {tag} bf16: worst rel_err / e_ref {worst[0]:.3f} at {worst[1]} ({worst[2]:.5f} / {worst[3]:.5f})")


def _run_trainer(model, args, batches, steps, fused, var_type="FIXED_LARGE"):
    ema_model = copy.deepcopy(model)
    if fused:
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule(args.path_type, 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType[var_type], loss_type=vaw_amd.LossType.MSE,
                                     rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, batches, Pbar())
    losses = [tr.train_step(s) for s in range(1, steps + 1)]
    psum = float(sum(p.double().abs().sum() for p in model.parameters()))
    esum = float(sum(v.double().abs().sum() for v in ema_model.state_dict().values()))
    return losses, psum, esum


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_trajectory_tiny_dit_fp32_vs_reference(fused):
    """6 optimizer steps of the reference Trainer on CPU (fixture) vs the HIP path in f32 parity mode with
    the CPU RNG stream injected.  north_star tolerance: 1e-4 relative on every per-step loss."""
    exp = load_json("trainer.json")["dit_tiny_latent"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, cpu_rng=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="fp32").to(DEV)
    losses, psum, esum = _run_trainer(model, args, synth_loader(8, 8, 8, 3, 10, latent=True), 6, fused)
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)
    assert psum == pytest.approx(exp["param_abs_sum"], rel=1e-5)
    assert esum == pytest.approx(exp["ema_abs_sum"], rel=1e-6)


def test_trainer_trajectory_tiny_dit_learned_variance_vs_reference():
    """learn_sigma=True + LEARNED_RANGE (loss = mse + vb): 6 reference steps, 1e-4 relative."""
    exp = load_json("trainer_vb.json")["dit_tiny_learn_sigma"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, cpu_rng=True, learn_sigma=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=True, compute_dtype="fp32").to(DEV)
    losses, psum, esum = _run_trainer(model, args, synth_loader(8, 8, 8, 3, 10, latent=True), 6, True, var_type="LEARNED_RANGE")
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)
    assert psum == pytest.approx(exp["param_abs_sum"], rel=1e-5)
    assert esum == pytest.approx(exp["ema_abs_sum"], rel=1e-6)


@pytest.mark.parametrize("loss", ["KL", "RESCALED_KL"])
def test_trainer_trajectory_kl_objective_vs_oracle_trainer(loss):
    """`--loss_type kl / rescaled_kl` with a learned variance through the Trainer (the terms dict then has no "mse" entry:
    reference tools/trainer.py:116 guards it): four steps of the HIP path in f32 against the oracle Trainer on the same CPU
    RNG stream, 1e-4 relative; the progress bar / last_mse bookkeeping must not trip over the missing key."""
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, cpu_rng=True, learn_sigma=True)
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.0, num_classes=10,
              learn_sigma=True)

    def run(pkg, diff_pkg, trainer_cls, dev, **mk):
        random.seed(42); np.random.seed(42); torch.manual_seed(42)
        model = pkg.DiT(**kw, **mk).to(dev)
        ema_model = copy.deepcopy(model)
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = diff_pkg.GaussianDiffusion(args=args, betas=diff_pkg.get_named_beta_schedule(args.path_type, 1000),
                                          model_mean_type=diff_pkg.ModelMeanType.EPSILON, model_var_type=diff_pkg.ModelVarType.LEARNED_RANGE,
                                          loss_type=diff_pkg.LossType[loss], rescale_timesteps=True)
        tr = trainer_cls(args, torch.device(dev), model, ema_model, opt, sched, diff, synth_loader(8, 8, 8, 3, 10, latent=True), Pbar())
        return [tr.train_step(s) for s in range(1, 5)]

    want = run(odit, od, otr.Trainer, "cpu")
    got = run(vaw_amd, vaw_amd, vaw_amd.Trainer, DEV, compute_dtype="fp32")
    assert all(np.isfinite(want)) and want[0] != want[-1]
    np.testing.assert_allclose(got, want, rtol=1e-4)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_ema_model_forward_follows_training(mode, fused):
    """The EMA copy is rewritten through raw pointers (fused AdamW+EMA kernel / ops.ema_update), which moves no parameter version:
    its bf16 shadow and fp8 weight copies must be dropped explicitly (FlatModule.mark_weights_changed), or an EMA model that was
    forwarded once keeps answering with the weights of that first forward (periodic sampling / evaluation during training, as the
    reference main loop does).  EMA forward, two training steps with a fast-moving average, EMA forward again: the second answer must
    match an f32 model carrying the current average within the mode's tolerance, and must differ from the first."""
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, class_dropout_prob=0.0, num_classes=10,
              learn_sigma=False)
    model = vaw_amd.DiT(**kw, compute_dtype=mode).to(DEV)
    with torch.no_grad():                                     # adaLN-Zero would make every output 0: move off the init
        for p_ in model.parameters():
            if p_.requires_grad:
                p_.add_(torch.randn_like(p_) * 0.05)
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=5e-2, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    decay = 0.5
    if fused:
        opt.attach_ema(ema_model, decay)
    B = 32
    x = torch.randn(B, 4, 8, 8, device=DEV)
    t = torch.rand(B, device=DEV) * 999.0
    y = torch.randint(0, 10, (B,), device=DEV)
    ema_model.eval()
    with torch.no_grad():
        out0 = ema_model(x, t, y)[0].clone()
    for _ in range(2):
        out, _ = model(x, t, y)
        (out.float() ** 2).mean().backward()
        opt.step()
        opt.zero_grad()
        if not fused:
            vaw_amd.ema(model, ema_model, decay)
    with torch.no_grad():
        out1 = ema_model(x, t, y)[0].clone()
    ref = vaw_amd.DiT(**kw, compute_dtype="fp32").to(DEV)
    ref.load_state_dict(ema_model.state_dict())
    ref.eval()
    with torch.no_grad():
        want = ref(x, t, y)[0]
    # rms error relative to the rms of the answer; a stale copy is off by the whole weight movement
    rms = lambda v: float(v.float().pow(2).mean().sqrt())
    e1, e0 = rms(out1 - want) / rms(want), rms(out0 - want) / rms(want)
    assert e1 < (0.03 if mode == "bf16" else 0.20), (e1, e0)      # (e4m3 on this tiny random model: 0.13; the stale copy: 0.91)
    assert e0 > 3 * e1, ("the average did not move enough for this test to mean anything", e1, e0)


def test_trainer_trajectory_dit_b4_fp32_vs_reference():
    """BASELINE config 4 (DiT-B/4 on 4x32x32 latents, 130 M parameters) at batch 8: 3 reference steps."""
    exp = load_json("trainer.json")["dit_b4_b8"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=32, cpu_rng=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=1000,
                          learn_sigma=False, compute_dtype="fp32").to(DEV)
    losses, psum, esum = _run_trainer(model, args, synth_loader(8, 8, 32, 3, 1000, latent=True), 3, True)
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)
    assert psum == pytest.approx(exp["param_abs_sum"], rel=1e-6)
    assert esum == pytest.approx(exp["ema_abs_sum"], rel=1e-7)


def test_dit_b4_bf16_tracks_fp32_and_grad_accum_and_clip():
    """Throughput mode at DiT-B/4: per-step losses within 2 % of the f32 reference trajectory (bf16 drift is
    reported, not hidden); gradient accumulation and clipping paths run."""
    exp = load_json("trainer.json")["dit_b4_b8"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=32, cpu_rng=True, amp=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=1000,
                          learn_sigma=False).to(DEV)
    losses, _, _ = _run_trainer(model, args, synth_loader(8, 8, 32, 3, 1000, latent=True), 3, True)
    np.testing.assert_allclose(losses, exp["losses"], rtol=2e-2)
    args2 = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=32, amp=True, grad_accumulation=2,
                      grad_clip=0.5)
    losses2, _, _ = _run_trainer(model, args2, synth_loader(8, 8, 32, 4, 1000, latent=True), 2, True)
    assert all(np.isfinite(losses2))


def test_full_batch_256_properties():
    """BASELINE size (DiT-B/4, batch 256, bf16): properties that need no oracle run.
    (1) per-sample independence: sample i's loss in the batch == its loss alone in a batch of 2;
    (2) determinism: same inputs -> bitwise same per-sample losses and gradients;
    (3) adaLN-Zero known answer at init: model output == 0, loss == w_t * mean(eps^2)."""
    torch.manual_seed(0)
    m = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=1000,
                      learn_sigma=False).to(DEV).train()
    args = base_args(in_chans=4, class_cond=True)
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE,
                                     rescale_timesteps=True)
    g = torch.Generator().manual_seed(1)
    B = 256
    x0 = (torch.randn(B, 4, 32, 32, generator=g) * 0.7).to(DEV)
    noise = torch.randn(B, 4, 32, 32, generator=g).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    y = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    terms = diff.training_losses(m, x0, None, t=t, model_kwargs={"y": y}, noise=noise)
    sig = torch.from_numpy(diff.sqrt_one_minus_alphas_cumprod).float().to(DEV)[t]
    torch.testing.assert_close(terms["mse"], sig * noise.pow(2).mean(dim=(1, 2, 3)), rtol=1e-5, atol=1e-6)
    perturb_(m, 5, std=0.02)
    t1 = diff.training_losses(m, x0, None, t=t, model_kwargs={"y": y}, noise=noise)
    t1["loss"].mean().backward()
    g1 = m.flat_grads().clone()
    m.zero_grad_flat()
    t2 = diff.training_losses(m, x0, None, t=t, model_kwargs={"y": y}, noise=noise)
    t2["loss"].mean().backward()
    assert torch.equal(t1["mse"], t2["mse"]) and torch.equal(g1, m.flat_grads())
    idx = torch.tensor([3, 200], device=DEV)
    sub = diff.training_losses(m, x0[idx], None, t=t[idx], model_kwargs={"y": y[idx]}, noise=noise[idx])
    torch.testing.assert_close(sub["mse"], t1["mse"][idx], rtol=1e-3, atol=1e-5)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0


def test_ddim_sampling_with_cfg_hip_dit_vs_oracle_dit():
    """Sampling side end to end: tiny DiT (class-conditional, null label) in eval mode under IntervalCFG, DDIM over a 12-step
    respaced process -- the HIP model + vaw_sample_step against the oracle model + the oracle's restated sampler, same
    weights, same CPU RNG stream, f32.  12 chained model calls: 1e-4 relative."""
    from oracle import diffusion as od, dit as odit, respace as orsp, sampler as osam
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.1,
              num_classes=10, learn_sigma=True)
    torch.manual_seed(3)
    om = odit.DiT(**kw)
    perturb_(om, 17)
    hm = vaw_amd.DiT(compute_dtype="fp32", **kw)
    hm.load_state_dict(om.state_dict())
    hm = hm.to(DEV).eval()
    om.eval()
    shape, y = (4, 4, 8, 8), torch.tensor([0, 3, 7, 9])
    res = []
    for pkg, sp, cfgc, model, dev, amod in ((od, orsp, osam.IntervalCFG, om, "cpu", od), (vaw_amd, vaw_amd, vaw_amd.IntervalCFG, hm, DEV, vaw_amd)):
        d = sp.SpacedDiffusion(use_timesteps=sp.space_timesteps(1000, "12"), args=base_args(learn_sigma=True, cpu_rng=True),
                               betas=pkg.get_named_beta_schedule("cosine", 1000), model_mean_type=amod.ModelMeanType.EPSILON,
                               model_var_type=amod.ModelVarType.LEARNED_RANGE, loss_type=amod.LossType.MSE, rescale_timesteps=True)
        cfg = cfgc(model, 10, 2.0, (-1.0, -1.0), True).eval()
        torch.manual_seed(77)
        out = d.ddim_sample_loop(cfg, shape, model_kwargs={"y": y.to(dev)}, device=dev, eta=0.3)
        res.append(out.cpu())
    torch.testing.assert_close(res[1], res[0], rtol=1e-4, atol=1e-4)
    assert float(res[0].abs().max()) > 0.1


def test_device_prefetcher_feeds_trainer():
    """Pinned host -> device copies on a side stream: same batches, same order, and the Trainer trajectory is unchanged."""
    cpu_batches = synth_loader(8, 8, 8, 3, 10, latent=True)
    pf = vaw_amd.DevicePrefetcher(cpu_batches, DEV, depth=2)
    for _ in range(2):
        got = list(pf)
        assert len(got) == len(cpu_batches)
        for (gx, gy), (x, y) in zip(got, cpu_batches):
            assert gx.is_cuda and torch.equal(gx.cpu(), x) and torch.equal(gy.cpu(), y)
    exp = load_json("trainer.json")["dit_tiny_latent"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, cpu_rng=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="fp32").to(DEV)
    losses, _, _ = _run_trainer(model, args, vaw_amd.DevicePrefetcher(synth_loader(8, 8, 8, 3, 10, latent=True), DEV), 6, True)
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)


def test_hip_graph_step_matches_eager_step():
    """args.hip_graph: the whole step (forward, loss, backward, clip, AdamW+EMA with a moving LR) captured once and replayed
    must reproduce the eager trajectory bit for bit when the random draws are pinned (fixed t / noise; the warm-up cosine
    schedule and Adam's bias corrections advance through the device-side hyper-parameters)."""
    class FixedDraws(vaw_amd.GaussianDiffusion):
        def training_losses(self, model, x_start, features=None, t=None, model_kwargs=None, noise=None):
            return super().training_losses(model, x_start, features, t=self._t, model_kwargs=model_kwargs, noise=self._noise)

    def run(graph):
        args = base_args(in_chans=4, class_cond=True, dataset="Pixels4", image_size=8, lr=1e-3, warmup_steps=3, cosine_decay=True,
                         total_steps=20, final_lr=1e-5, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph)
        args.in_chans = 3            # no latent sampling: Trainer draws nothing itself
        random.seed(42); np.random.seed(42); torch.manual_seed(42)
        model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                            class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="bf16").to(DEV)
        perturb_(model, 5)
        ema_model = copy.deepcopy(model)
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = FixedDraws(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                          model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        g = torch.Generator().manual_seed(9)
        diff._t = torch.randint(0, 1000, (8,), generator=g).to(DEV)
        diff._noise = torch.randn(8, 4, 8, 8, generator=g).to(DEV)
        batches = [(torch.randn(8, 4, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
        tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, batches, Pbar())
        losses = [float(tr.train_step(s)) for s in range(1, 9)]
        return losses, model._flat.clone(), ema_model._flat.clone(), sched.get_last_lr()[0], opt.step_count

    le, pe, ee, lre, ne = run(False)
    lg, pg, eg, lrg, ng = run(True)
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(ee, eg)
    assert lre == lrg and ne == ng == 8
    assert le[-1] < le[0]


def test_backward_stage_hooks_and_early_adaln_bucket():
    """With a gradient-ready listener (DDP) the backward reports head, blocks L-1..0, an early bucket with the adaLN rows of
    the upper half of the blocks, then the rest; the stage ranges tile the flat gradient buffer exactly once and the
    gradients are the same as without a listener (the packed adaLN weight gradient is then one GEMM instead of two)."""
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=4, num_heads=2, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=False, compute_dtype="fp32")
    torch.manual_seed(5)
    m = vaw_amd.DiT(**kw)
    perturb_(m, 6)
    m = m.to(DEV)
    m.ensure_flat()
    g = torch.Generator().manual_seed(1)
    x, t, y = torch.randn(4, 4, 8, 8, generator=g).to(DEV), torch.rand(4, generator=g).to(DEV) * 999, torch.randint(0, 10, (4,), generator=g).to(DEV)
    gout = torch.randn(4, 4, 8, 8, generator=g).to(DEV)

    def grads(hook):
        m.grad_ready_hook = hook
        m.zero_grad_flat()
        out, _ = m(x, t, y)
        (out * gout).sum().backward()
        return m.flat_grads().clone()

    ref = grads(None)
    seen = []
    got = grads(seen.append)
    m.grad_ready_hook = None
    assert seen == [5, 4, 3, "ada_hi", 2, 1, 0], seen          # block l reports stage l+1; blocks 3 and 2 are the upper half
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-7)
    cover = torch.zeros(m._flat_n_train, dtype=torch.int32)
    for stage, rng in m.grad_stage_bounds().items():
        for lo, hi in (rng if isinstance(rng, list) else [rng]):
            cover[lo:hi] += 1
    assert int(cover.min()) == 1 and int(cover.max()) == 1


def test_trainer_with_loss_second_moment_sampler():
    """args.schedule_sampler="loss-second-moment" (the wiring the reference's Trainer lacks): t comes from the sampler, the
    per-sample losses feed its history, the importance weights multiply the loss; after enough steps on a 20-step
    process the sampler is warmed up and its weights are no longer uniform."""
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, schedule_sampler="loss-second-moment")
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="fp32").to(DEV)
    perturb_(model, 2)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("linear", 20), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, None, opt, sched, diff, synth_loader(8, 8, 8, 3, 10, latent=True), Pbar())
    assert isinstance(tr.schedule_sampler, vaw_amd.LossSecondMomentResampler)
    assert np.allclose(tr.schedule_sampler.weights(), 1.0)              # not warmed up: uniform
    losses = [tr.train_step(s) for s in range(1, 61)]
    assert all(np.isfinite(losses))
    w = tr.schedule_sampler.weights()
    assert tr.schedule_sampler._warmed_up() and abs(w.sum() - 1.0) < 1e-9 and w.std() > 0


@pytest.mark.parametrize("wrapped", [False, True])
def test_checkpoint_resume_hip_dit_fused_adamw_is_bitwise(tmp_path, wrapped):
    """Reference checkpoint dict {'model','optimizer','step','ema_model'} (tools/utils.py:93-120) on the real path: 3 steps of
    a HIP DiT (bf16 kernels, flat storage) + FusedAdamW + EMA, save, FRESH objects, load, 3 more steps == 6 uninterrupted
    steps, bit for bit (losses, parameters, EMA, both Adam moments).  wrapped: through vaw_amd.DistributedDataParallel, whose
    state_dict carries the 'module.' prefix like torch DDP's; the checkpoint is then loaded into a bare model and vice versa.
    The optimizer entry is in torch.optim.AdamW's own format, indexed like AdamW(model.parameters())."""
    import os
    import socket
    import torch.distributed as dist
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=False, compute_dtype="bf16")
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, amp=True, cpu_rng=True, warmup_steps=2,
                     cosine_decay=True, total_steps=20, final_lr=1e-5, logdir=str(tmp_path), model="DiT-tiny", mean_type="EPSILON")
    batches = synth_loader(8, 8, 8, 3, 10, latent=True)
    started = False
    if wrapped:
        sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        vaw_amd.dist_util.setup_dist(backend="gloo", device_index=0)
        started = True

    def fresh(wrap):
        torch.manual_seed(5)
        model = vaw_amd.DiT(**kw)
        perturb_(model, 9)
        model = model.to(DEV)
        ema_model = copy.deepcopy(model)
        net = vaw_amd.DistributedDataParallel(model) if wrap else model
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                         model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                         loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        tr = vaw_amd.Trainer(args, torch.device(DEV), net, ema_model, opt, sched, diff, batches, Pbar())
        return model, net, ema_model, opt, sched, tr

    def steps(tr, first, n):
        out = []
        for s in range(first, first + n):
            torch.manual_seed(1000 + s)           # the CPU RNG stream of step s (noise, t, latent sampling)
            out.append(tr.train_step(s))
        return out

    try:
        model_a, _, ema_a, opt_a, _, tr_a = fresh(wrapped)
        ref = steps(tr_a, 1, 6)
        model_b, net_b, ema_b, opt_b, sched_b, tr_b = fresh(wrapped)
        first = steps(tr_b, 1, 3)
        path = vaw_amd.save_checkpoint(args, 3, net_b, opt_b, ema_model=ema_b, scheduler=sched_b)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        assert set(ck) == {"model", "optimizer", "step", "ema_model", "scheduler"}
        assert all(k.startswith("module.") for k in ck["model"]) == wrapped
        n_train = sum(1 for p in model_b.parameters() if p.requires_grad)
        assert len(ck["optimizer"]["state"]) == n_train and len(ck["optimizer"]["param_groups"][0]["params"]) == len(list(model_b.parameters()))
        # the optimizer entry loads into a stock torch AdamW over the same parameters (reference main.py:354)
        stock = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in model_b.parameters()], lr=1e-3)
        stock.load_state_dict(ck["optimizer"])
        del model_b, net_b, ema_b, opt_b, sched_b, tr_b
        model_c, net_c, ema_c, opt_c, sched_c, tr_c = fresh(wrapped)
        with torch.no_grad():                      # make sure nothing survives from the constructor
            model_c.flat_params().add_(1.0)
            ema_c.flat_params().mul_(0.0)
        got = vaw_amd.load_checkpoint(path, model=net_c, optimizer=opt_c, ema_model=ema_c, scheduler=sched_c)
        assert got["step"] == 3 and opt_c.step_count == 3
        second = steps(tr_c, 4, 3)
        assert first + second == ref
        for (k, v), (_, w) in zip(model_c.state_dict().items(), model_a.state_dict().items()):   # (the flat buffers also hold
            assert torch.equal(v, w), k                                                            # alignment gaps: compare entries)
        for (k, v), (_, w) in zip(ema_c.state_dict().items(), ema_a.state_dict().items()):
            assert torch.equal(v, w), k
        assert torch.equal(opt_c.exp_avg, opt_a.exp_avg) and torch.equal(opt_c.exp_avg_sq, opt_a.exp_avg_sq)
        if wrapped:      # cross-loading: the 'module.'-prefixed checkpoint into a bare model
            model_d = fresh(False)[0]
            vaw_amd.load_checkpoint(path, model=model_d)
            for k, v in model_d.state_dict().items():
                assert torch.equal(v.cpu(), ck["model"]["module." + k]), k
    finally:
        if started:
            vaw_amd.dist_util.cleanup_dist()


def test_edm_heun_sampling_hip_dit_vs_oracle_dit():
    """EDM Heun sampler (vaw_amd.edm_sample over vaw_amd.EDMDenoiser) with the HIP DiT in eval mode under IntervalCFG vs the same
    sampler code over the oracle DiT on the CPU: same weights, same CPU RNG stream, f32 kernels; 2 x 7 - 1 chained model calls."""
    from oracle import dit as odit, sampler as osam
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.1,
              num_classes=10, learn_sigma=False)
    torch.manual_seed(3)
    om = odit.DiT(**kw)
    perturb_(om, 17)
    hm = vaw_amd.DiT(compute_dtype="fp32", **kw)
    hm.load_state_dict(om.state_dict())
    hm, om = hm.to(DEV).eval(), om.eval()
    lat = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    y = torch.tensor([0, 3, 7, 9])
    outs = []
    for model, cfgc, dev in ((om, osam.IntervalCFG, "cpu"), (hm, vaw_amd.IntervalCFG, DEV)):
        net = vaw_amd.EDMDenoiser(cfgc(model, 10, 1.7, (-1.0, -1.0), True).eval(), img_resolution=8, img_channels=4, label_dim=10,
                                  pred_type="EPSILON", noise_schedule="cosine").to(dev)
        torch.manual_seed(11)
        rl = lambda t: torch.randn(t.shape, dtype=t.dtype).to(t.device)          # CPU stream for both
        outs.append(vaw_amd.edm_sample(net, lat.to(dev), class_labels=y.to(dev), num_steps=7, solver="heun", S_churn=2.0, randn_like=rl).cpu())
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-4, atol=1e-4)


def test_bias_gradient_fold_follows_the_producers_row_counts():
    """The bias gradients of the blocks are folded from partial column sums whose ROW COUNT depends on the kernel each producer
    ran on (one row per 64 / 128 / 256 rows of C for the GEMMs, per 64 / 128 / 256 query rows for the attention backward), and
    that choice can change between two backwards of ONE workspace (CUs reserved for a collective, vaw_debug_gemm_tile,
    VAW_ATTN_BWD_BIG).  The device table of the batched fold bakes the counts in: it has to be rebuilt when they move.  Two
    backwards of one model under two settings must each give the bias gradients of a fresh model run under that setting."""
    import os
    from vaw_amd._lib import lib

    def make():
        torch.manual_seed(5)
        m = vaw_amd.DiT(image_size=32, patch_size=2, in_channels=4, hidden_size=256, depth=2, num_heads=4, num_classes=10,
                        class_dropout_prob=0.0, learn_sigma=False, compute_dtype="bf16").to(DEV).train()
        perturb_(m, 3, 0.05)
        m.ensure_flat()
        return m

    g = torch.Generator().manual_seed(9)
    x = torch.randn(16, 4, 32, 32, generator=g).to(DEV)           # 16 x 256 tokens = 4096 rows
    t = (torch.rand(16, generator=g) * 999).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    gout = torch.randn(16, 4, 32, 32, generator=g).to(DEV)

    def backward(m, tile, attn):
        lib().vaw_debug_gemm_tile(tile)
        os.environ["VAW_ATTN_BWD_BIG"] = attn
        try:
            m.zero_grad_flat()
            out, _ = m(x, t, y)
            (out * gout).sum().backward()
            torch.cuda.synchronize()
            return {k: p.grad.clone() for k, p in m.named_parameters() if k.endswith("bias") and p.grad is not None}
        finally:
            lib().vaw_debug_gemm_tile(-1)
            os.environ.pop("VAW_ATTN_BWD_BIG", None)

    settings = [(0, "0"), (6, "2"), (2, "1"), (0, "0")]            # 128-row tiles / 64-row ring / 256-row persistent; three attention families
    shared = make()
    for tile, attn in settings:
        got = backward(shared, tile, attn)
        ref = backward(make(), tile, attn)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (tile, attn, k, float((got[k] - ref[k]).abs().max()))

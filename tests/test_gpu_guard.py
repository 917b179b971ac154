"""The step guard on the GPU (csrc/guard.hip, the guarded AdamW + EMA pass of csrc/elementwise.hip, vaw_amd.StepGuard,
FusedAdamW.attach_guard, Trainer's args.skip_nonfinite): a refused step leaves every optimizer stream bit for bit as it was, an
accepted one is bit for bit the unguarded step, the verdict follows the float64 restatement of tests/guard_cases.py, and the
trainer survives a poisoned batch in bf16, fp32 and fp8, eagerly, inside a replayed hipGraph and with the sharded optimizer.
Tiny shapes throughout.  Run on the MI355X box: pytest -m gpu."""
import copy
import itertools
import os
import random
import socket
import sys
import traceback
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO, Pbar, base_args, perturb_

import guard_cases as gc

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops

DEV = "cuda"
# two full tiles of ADAM_U x 256 float4 (4096 elements each), a partial tile of 37 float4 and an n % 4 tail of 3
N = 2 * 4096 + 4 * 37 + 3
PAD = 64                       # canary elements behind every stream
HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, step=3, decay=0.999, clip=0.5)
FLAGS = list(itertools.product((False, True), repeat=4))          # ema, shadow, clip, zero_grad


def _streams(seed=0):
    """p, g, m, v, ema (f32) and the bf16 shadow, each N elements at the head of an N + PAD buffer whose tail is a canary"""
    gen = torch.Generator().manual_seed(seed)
    s = {k: torch.randn(N + PAD, generator=gen) for k in ("p", "g", "m", "e")}
    s["v"] = torch.rand(N + PAD, generator=gen) * 1e-2
    s["m"] *= 0.1
    s = {k: t.to(DEV) for k, t in s.items()}
    s["sh"] = s["p"].to(torch.bfloat16) + 1          # (stale on purpose: the pass must overwrite it)
    return s


def _launch(s, ema, shadow, clip, zero_grad, entry, ok):
    """one AdamW + EMA pass over the first N elements of the streams `s`, through the host-scalar or the _dev entry; ok: None for
    the unguarded entry, else the device verdict"""
    sumsq = torch.zeros(1, device=DEV)
    if clip:
        ops.sumsq(s["g"][:N], sumsq)
    hyper = None
    if entry == "dev":
        hyper = torch.tensor([HP["lr"], 1.0 - HP["b1"] ** HP["step"], 1.0 - HP["b2"] ** HP["step"], 0.0], device=DEV)
    kw = {} if ok is None else {"ok": ok}
    ops.adamw_ema_step(s["p"][:N], s["g"][:N], s["m"][:N], s["v"][:N], s["e"][:N] if ema else None, s["sh"][:N] if shadow else None,
                       HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], HP["step"], HP["decay"], sumsq if clip else None,
                       HP["clip"] if clip else None, zero_grad, hyper=hyper, **kw)


def _clone(s):
    return {k: t.clone() for k, t in s.items()}


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_guarded_pass_with_ok_1_is_bitwise_the_unguarded_pass(entry):
    """every combination of ema / shadow / clip / zero_grad: all six streams, canaries included, equal the unguarded entry's"""
    ok = torch.ones(1, dtype=torch.int32, device=DEV)
    start = _streams()
    for ema, shadow, clip, zg in FLAGS:
        ref, got = _clone(start), _clone(start)
        _launch(ref, ema, shadow, clip, zg, entry, None)
        _launch(got, ema, shadow, clip, zg, entry, ok)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (k, ema, shadow, clip, zg)
        # ... and the pass did something: the weights moved, the canaries did not
        assert not torch.equal(got["p"][:N], start["p"][:N]) and torch.equal(got["p"][N:], start["p"][N:])
        assert bool((got["g"][:N] == 0).all()) == zg
    assert int(ok.item()) == 1


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_guarded_pass_with_ok_0_touches_nothing_but_the_gradient(entry):
    """p, m, v, ema and shadow bitwise untouched; g zero exactly when zero_grad (and untouched otherwise)"""
    ok = torch.zeros(1, dtype=torch.int32, device=DEV)
    start = _streams(1)
    start["g"][5] = float("nan")                    # what a refused step looks like: nothing of it may reach a stream
    start["g"][N - 1] = float("inf")
    for ema, shadow, clip, zg in FLAGS:
        got = _clone(start)
        _launch(got, ema, shadow, clip, zg, entry, ok)
        for k in ("p", "m", "v", "e", "sh"):
            assert torch.equal(got[k].view(torch.int32 if got[k].dtype == torch.float32 else torch.int16),
                               start[k].view(torch.int32 if start[k].dtype == torch.float32 else torch.int16)), (k, ema, shadow, clip, zg)
        if zg:
            assert bool((got["g"][:N] == 0).all())
        else:
            assert torch.equal(got["g"][:N].view(torch.int32), start["g"][:N].view(torch.int32))
        assert torch.equal(got["g"][N:], start["g"][N:])
    assert int(ok.item()) == 0


def test_step_guard_kernel_follows_the_restatement_launch_by_launch():
    """the CPU test's sequence, one launch at a time: counters exactly, statistics to 1e-12 relative (float64, a handful of
    operations; inf and NaN norms compare as such)"""
    want = gc.guard_reference([s for s, _, _ in gc.SEQUENCE], **gc.SPIKE)
    guard = vaw_amd.StepGuard(DEV, **gc.SPIKE)
    assert guard.counters() == dict.fromkeys(gc.COUNTERS, 0)
    sumsq = torch.zeros(1, device=DEV)
    for (ss, verdict, why), (wc, ws) in zip(gc.SEQUENCE, want):
        sumsq.fill_(ss)
        guard.check(sumsq)
        c, s = guard.counters(), guard.stats()
        print(why, c, s)
        assert c == wc and c["ok"] == verdict and int(guard.ok.item()) == verdict, (why, c, wc)
        for k in gc.STATS:
            np.testing.assert_allclose(s[k], ws[k], rtol=1e-12, atol=0, err_msg=f"{why}: {k}")
    # the state moves to a new guard, which goes on as the old one would
    sd = guard.state_dict()
    other = vaw_amd.StepGuard(DEV, **gc.SPIKE)
    other.load_state_dict(sd)
    for g in (guard, other):
        sumsq.fill_(1.0e6)
        g.check(sumsq)
    assert other.counters() == guard.counters() and other.stats() == guard.stats() and other.counters()["skipped_spike"] == 3
    # no factor: only non-finite sums are refused
    plain = vaw_amd.StepGuard(DEV)
    for ss in (1.0, 1.0e30, float("inf")):
        sumsq.fill_(ss)
        plain.check(sumsq)
    assert plain.counters() == dict(ok=0, steps=3, applied=2, skipped_nonfinite=1, skipped_spike=0, in_a_row=1)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", [0, 2 * 4096 + 4 * 11 + 1, N - 1], ids=["first", "partial_tile", "tail"])
def test_sumsq_guard_update_chain_refuses_a_bad_element_wherever_it_sits(where, bad):
    """vaw_sumsq -> vaw_step_guard -> guarded pass on raw streams of N elements: the only place an n % 4 tail exists (a model's flat
    gradient is padded to 64 elements)."""
    guard = vaw_amd.StepGuard(DEV)
    start = _streams(2)
    start["g"][where] = bad
    got = _clone(start)
    sumsq = torch.zeros(1, device=DEV)
    ops.sumsq(got["g"][:N], sumsq)
    guard.check(sumsq)
    ops.adamw_ema_step(got["p"][:N], got["g"][:N], got["m"][:N], got["v"][:N], got["e"][:N], got["sh"][:N], HP["lr"], HP["b1"], HP["b2"],
                       HP["eps"], HP["wd"], HP["step"], HP["decay"], sumsq, HP["clip"], False, ok=guard.ok)
    for k in ("p", "m", "v", "e", "sh"):
        assert torch.equal(got[k], start[k]), k
    assert guard.counters() == dict(ok=0, steps=1, applied=0, skipped_nonfinite=1, skipped_spike=0, in_a_row=1)


def test_fp8_scale_update_finite_keeps_the_scale_of_an_overflowed_tensor():
    st = ops.fp8_states([vaw_amd._lib.FP8, vaw_amd._lib.BF8, vaw_amd._lib.FP8, vaw_amd._lib.FP8, vaw_amd._lib.BF8], DEV)
    st[:, 0] = torch.tensor([0.5, 0.25, 2.0, 4.0, 8.0])
    st[:, 1] = torch.tensor([3.0, float("inf"), 0.0, float("nan"), 1.0e38])
    plain, finite = st.clone(), st.clone()
    ops.fp8_scale_update(plain)
    ops.fp8_scale_update(finite, finite=True)
    assert bool((plain[:, 1] == 0).all()) and bool((finite[:, 1] == 0).all())          # the max is cleared either way
    assert torch.equal(finite[:, 2:], st[:, 2:])
    assert torch.equal(finite[[0, 2, 3, 4], 0], plain[[0, 2, 3, 4], 0])                # finite maxima: the plain update, bit for bit
    assert float(finite[0, 0]) == float(np.float32(3.0) / np.float32(st[0, 2].item()))      # running max / (FMAX / margin), in f32
    assert float(finite[2, 0]) == 2.0 and float(finite[3, 0]) == 4.0                    # zero and NaN: kept, as they always were
    assert float(finite[4, 0]) == float(np.float32(1.0e38) / np.float32(st[4, 2].item()))
    assert float(finite[1, 0]) == 0.25                                                  # inf: the scale in use stays ...
    assert torch.isinf(plain[1, 0])                                                     # ... where the plain update makes it infinite


def _diffusion(args, cls=None):
    return (cls or vaw_amd.GaussianDiffusion)(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                              model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                              loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)


def test_resampler_update_finite_counts_bad_losses_and_records_none_of_them():
    """what Trainer switches the device sampler to: pairs with a NaN or inf loss are counted in invalid_count() and never reach the
    history; on finite losses the update is the plain one bit for bit.  (Without the switch the same pairs make weights() NaN:
    the behaviour the guard's runs must not meet.)"""
    d = SimpleNamespace(num_timesteps=70, args=SimpleNamespace())
    plain = vaw_amd.DeviceLossSecondMomentResampler(d, DEV, history_per_term=3)
    finite = vaw_amd.DeviceLossSecondMomentResampler(d, DEV, history_per_term=3)
    finite.skip_nonfinite = True
    gen = torch.Generator().manual_seed(3)
    ts = torch.arange(70).repeat(3)[torch.randperm(210, generator=gen)].to(DEV)
    losses = torch.rand(210, generator=gen).to(DEV) + 0.1
    for s in (plain, finite):
        s.update_with_all_losses(ts, losses)
    assert torch.equal(plain.ring, finite.ring) and torch.equal(plain.seen, finite.seen) and finite.invalid_count() == 0
    assert int(finite.seen.min()) == 3                                                   # warm: p comes from the history now
    w0 = finite.weights()
    ts2 = torch.tensor([5, 5, 7, 69, 69, 70], device=DEV)
    bad = torch.tensor([float("nan"), 1.5, float("inf"), float("-inf"), 0.5, float("nan")], device=DEV)
    for s in (plain, finite):
        s.update_with_all_losses(ts2, bad)
    assert finite.invalid_count() == 4                                                   # two NaN (one of them also out of range), +inf, -inf
    assert bool(torch.isfinite(finite.ring).all()) and np.isfinite(finite.weights()).all()
    assert finite.seen.tolist() == [3 + (t in (5, 69)) for t in range(70)]
    assert not np.array_equal(finite.weights(), w0)
    assert plain.invalid_count() == 1 and not np.isfinite(plain.weights()).all()


# ---- FusedAdamW.attach_guard on a model ---------------------------------------------------------------------------------------
KW = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.0, num_classes=10,
          learn_sigma=False)
_OPT = {}


def _guarded_optimizer():
    """tiny bf16 DiT with an EMA copy, a FusedAdamW with the EMA folded in and a guard attached, after one clean step; shared by
    the cases below (each of them snapshots the state it starts from)"""
    if not _OPT:
        torch.manual_seed(5)
        model = vaw_amd.DiT(compute_dtype="bf16", **KW)
        perturb_(model, 6)
        model = model.to(DEV).train()
        ema_model = copy.deepcopy(model)
        opt = vaw_amd.FusedAdamW(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01)
        opt.attach_ema(ema_model, 0.999)
        guard = vaw_amd.StepGuard(DEV)
        opt.attach_guard(guard)
        model.shadow_bf16()
        gen = torch.Generator().manual_seed(8)
        model.flat_grads().copy_(torch.randn(model._flat_n_train, generator=gen) * 1e-2)
        opt.step()
        _OPT.update(model=model, ema=ema_model, opt=opt, guard=guard, gen=gen)
    return _OPT


@pytest.mark.parametrize("clip", [None, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first", "partial_tile", "last"])
def test_optimizer_step_skips_a_bad_gradient_wherever_it_sits(where, bad, clip):
    """model._flat, both moments, the EMA model's trainable range and the bf16 shadow are bitwise unchanged and one skip is counted;
    the next clean step is applied.  (flat_grads() is padded to a multiple of 64: its last element stands for the n % 4 tail,
    which test_sumsq_guard_update_chain_refuses_a_bad_element_wherever_it_sits covers on raw streams.  The EMA of the frozen
    entries behind the trainable range runs on a skipped step as on any other, by design.)"""
    o = _guarded_optimizer()
    model, ema_model, opt, guard = o["model"], o["ema"], o["opt"], o["guard"]
    n = model._flat_n_train
    assert n > 4096 and n % 4096 != 0, n                      # full tiles and a partial one
    at = {"first": 0, "partial_tile": n // 4096 * 4096 + 4 * 3 + 2, "last": n - 1}[where]
    opt.max_grad_norm = clip
    g = model.flat_grads()
    g.copy_(torch.randn(n, generator=o["gen"]) * 1e-2)
    g[at] = bad
    before = dict(flat=model._flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), ema=ema_model._flat[:n].clone(),
                  shadow=model._flat_shadow.clone())
    c0, steps0 = guard.counters(), opt.step_count
    opt.step()
    now = dict(flat=model._flat, m=opt.exp_avg, v=opt.exp_avg_sq, ema=ema_model._flat[:n], shadow=model._flat_shadow)
    for k in before:
        assert torch.equal(before[k], now[k]), k
    c1 = guard.counters()
    assert c1["skipped_nonfinite"] == c0["skipped_nonfinite"] + 1 and c1["applied"] == c0["applied"] and c1["ok"] == 0
    assert c1["in_a_row"] == c0["in_a_row"] + 1 and opt.step_count == steps0 + 1          # the host's step count advances
    g.copy_(torch.randn(n, generator=o["gen"]) * 1e-2)
    opt.step()
    c2 = guard.counters()
    assert c2["applied"] == c1["applied"] + 1 and c2["in_a_row"] == 0 and c2["ok"] == 1
    assert not torch.equal(before["flat"], model._flat) and bool(torch.isfinite(model._flat).all())
    opt.max_grad_norm = None


# ---- Trainer ------------------------------------------------------------------------------------------------------------------
class FixedDraws(vaw_amd.GaussianDiffusion):
    """t and noise pinned, so that eager and captured runs, guarded and unguarded ones, see the same draws"""

    def training_losses(self, model, x_start, features=None, t=None, model_kwargs=None, noise=None):
        return super().training_losses(model, x_start, features, t=self._t, model_kwargs=model_kwargs, noise=self._noise)


_TRAIN = {}


def _train(dtype, guard, poison=(), steps=6, graph=False, hidden=64, batch=4, **extra):
    """`steps` trainer steps of a tiny DiT (image 8, patch 2, depth 2) from fixed seeds; the batches of the (1-based) steps in
    `poison` carry one NaN pixel.  Computed once per configuration and shared, never modified."""
    key = (dtype, guard, tuple(poison), steps, graph, hidden, batch, tuple(sorted(extra.items())))
    if key in _TRAIN:
        return _TRAIN[key]
    args = base_args(in_chans=4, class_cond=True, dataset="Pixels4", image_size=8, lr=1e-3, warmup_steps=3, cosine_decay=True,
                     total_steps=20, final_lr=1e-5, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph, amp=dtype != "fp32", **extra)
    args.in_chans = 3            # no latent sampling: Trainer draws nothing itself
    if guard:
        args.skip_nonfinite = True
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(compute_dtype=dtype, **dict(KW, hidden_size=hidden)).to(DEV)
    perturb_(model, 5)
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = _diffusion(args, FixedDraws)
    g = torch.Generator().manual_seed(9)
    diff._t = torch.randint(0, 1000, (batch,), generator=g).to(DEV)
    diff._noise = torch.randn(batch, 4, 8, 8, generator=g).to(DEV)
    batches = [(torch.randn(batch, 4, 8, 8, generator=g), torch.randint(0, 10, (batch,), generator=g)) for _ in range(steps)]
    for s in poison:
        batches[s - 1][0][1, 2, 3, 4] = float("nan")
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, batches, Pbar())
    assert (tr.guard is not None) == guard and (opt.guard is tr.guard)
    losses, flats, emas = [], [], []
    n = model._flat_n_train
    for s in range(1, steps + 1):
        losses.append(float(tr.train_step(s)))          # (read at once: a replayed graph hands back the same tensor every step)
        flats.append(model._flat.clone())
        emas.append(ema_model._flat[:n].clone())
    assert (tr._graph is not None) == bool(graph)
    out = _TRAIN[key] = dict(losses=[float(x) for x in losses], flats=flats, emas=emas, m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                             ema_full=ema_model._flat.clone(), counters=tr.guard.counters() if guard else None, model=model, trainer=tr,
                             steps=opt.step_count, lr=sched.get_last_lr()[0])
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_trainer_skips_the_poisoned_step_and_goes_on(dtype):
    r = _train(dtype, True, poison=(3,))
    assert torch.equal(r["flats"][2], r["flats"][1]) and torch.equal(r["emas"][2], r["emas"][1])
    assert not torch.equal(r["flats"][1], r["flats"][0])
    for s in (3, 4, 5):                                       # steps 4-6 move the weights again
        assert not torch.equal(r["flats"][s], r["flats"][s - 1]) and not torch.equal(r["emas"][s], r["emas"][s - 1])
    for t in r["flats"] + r["emas"] + [r["m"], r["v"], r["ema_full"]]:
        assert bool(torch.isfinite(t).all())
    assert not np.isfinite(r["losses"][2]) and np.isfinite(r["losses"][:2] + r["losses"][3:]).all()
    c = r["counters"]
    assert (c["skipped_nonfinite"], c["applied"], c["in_a_row"], c["steps"], c["skipped_spike"]) == (1, 5, 0, 6, 0)
    assert r["steps"] == 6                                    # the Adam step count and the LR schedule advanced on the skipped step
    assert r["lr"] == _train(dtype, True)["lr"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_attached_guard_is_bitwise_neutral_on_clean_batches(dtype):
    on, off = _train(dtype, True), _train(dtype, False)
    assert on["losses"] == off["losses"]
    for k in ("m", "v", "ema_full"):
        assert torch.equal(on[k], off[k]), k
    for a, b in zip(on["flats"], off["flats"]):
        assert torch.equal(a, b)
    assert on["counters"] == dict(ok=1, steps=6, applied=6, skipped_nonfinite=0, skipped_spike=0, in_a_row=0)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_without_the_guard_one_poisoned_batch_ends_the_run(dtype):
    """The behaviour the feature exists to prevent, stated as such: with the guard absent the poisoned step writes NaN into the
    masters, both moments and the EMA, and every later step keeps them there."""
    r = _train(dtype, False, poison=(3,))
    for t in (r["flats"][-1], r["m"], r["v"], r["emas"][-1]):
        assert not bool(torch.isfinite(t).all())
    assert bool(torch.isfinite(r["flats"][1]).all()) and not np.isfinite(r["losses"][3:]).any()


def test_fp8_scales_survive_the_poisoned_step():
    """the dit_fp8_delayed shape of tests/model_grad_cases.py (hidden 128, batch 16): after the skip every delayed-scaling state is
    finite and positive, and the next step's loss is finite"""
    r = _train("fp8", True, poison=(3,), hidden=128, batch=16)
    model = r["model"]
    assert model.fp8_finite_scales and model.compute_dtype == "fp8" and model._ws_cur.fp8
    for st in (model._ws_cur.fp8_states, model._fp8_wstates):
        assert bool(torch.isfinite(st[:, 0]).all()) and bool((st[:, 0] > 0).all()), st[:, :2]
    assert torch.equal(r["flats"][2], r["flats"][1]) and not torch.equal(r["flats"][3], r["flats"][2])
    assert not np.isfinite(r["losses"][2]) and np.isfinite(r["losses"][3:]).all(), r["losses"]
    assert bool(torch.isfinite(r["flats"][-1]).all())
    c = r["counters"]
    assert (c["skipped_nonfinite"], c["applied"], c["in_a_row"]) == (1, 5, 0)


def test_hip_graph_replay_skips_the_poisoned_step_like_the_eager_run():
    """args.hip_graph with defer_loss_sync: steps 1-2 run eagerly, step 3 captures, the poisoned batch arrives on replayed step 5;
    the verdict, the skip and everything after it are bitwise the eager guarded run's"""
    eager, graph = _train("bf16", True, poison=(5,), steps=7), _train("bf16", True, poison=(5,), steps=7, graph=True)
    assert graph["trainer"]._graph is not None and eager["trainer"]._graph is None
    assert [np.float32(x).tobytes() for x in graph["losses"]] == [np.float32(x).tobytes() for x in eager["losses"]]
    for a, b in zip(graph["flats"] + graph["emas"], eager["flats"] + eager["emas"]):
        assert torch.equal(a, b)
    for k in ("m", "v", "ema_full"):
        assert torch.equal(graph[k], eager[k]), k
    assert torch.equal(graph["flats"][4], graph["flats"][3]) and not torch.equal(graph["flats"][5], graph["flats"][4])
    assert graph["counters"] == eager["counters"] == dict(ok=1, steps=7, applied=6, skipped_nonfinite=1, skipped_spike=0, in_a_row=0)


def test_trainer_switches_the_device_sampler_and_gives_up_after_too_many_skips():
    """args.schedule_sampler = "loss-second-moment-device" behind the guard records no NaN loss; with max_consecutive_skips = 2 and
    guard_check_every = 1 the second poisoned batch in a row raises FloatingPointError naming the step"""
    args = base_args(in_chans=4, class_cond=True, dataset="Pixels4", image_size=8, lr=1e-3, total_steps=20, amp=True,
                     schedule_sampler="loss-second-moment-device", skip_nonfinite=True, max_consecutive_skips=2, guard_check_every=1)
    args.in_chans = 3
    torch.manual_seed(1)
    model = vaw_amd.DiT(compute_dtype="bf16", **KW).to(DEV)
    perturb_(model, 5)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(4, 4, 8, 8, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(4)]
    for i in (1, 2):
        batches[i][0][0, 0, 0, 0] = float("nan")
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, copy.deepcopy(model), opt, sched, _diffusion(args), batches, Pbar())
    assert tr.schedule_sampler.skip_nonfinite and tr.guard is not None
    assert np.isfinite(tr.train_step(1))
    start = model._flat.clone()
    assert not np.isfinite(tr.train_step(2))                  # one skip: below the limit
    with pytest.raises(FloatingPointError, match=r"step 3\b.*2 updates in a row"):
        tr.train_step(3)
    assert torch.equal(model._flat, start)
    assert tr.schedule_sampler.invalid_count() == 2           # one NaN loss per poisoned batch, none of them in the history
    assert bool(torch.isfinite(tr.schedule_sampler.ring).all()) and np.isfinite(tr.schedule_sampler.weights()).all()
    assert tr.guard.counters()["in_a_row"] == 2


# ---- sharded optimizer (child processes: a process group lives for the life of a process) ---------------------------------------
# DistributedDataParallel(shard_optimizer=True) shards only when world > 1 (at world 1 it is the plain optimizer, which the tests
# above cover), so FusedAdamW._step_sharded is reached the way tests/test_gpu_dist.py reaches it: two ranks on the one GPU over gloo.
def _sharded_worker(rank, world, port, q):
    try:
        sys.path.insert(0, REPO)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import vaw_amd
        vaw_amd.dist_util.setup_dist(backend="gloo", device_index=0)
        torch.manual_seed(21)
        model = vaw_amd.DiT(compute_dtype="fp32", **dict(KW, depth=4))
        perturb_(model, 31)
        model = model.to(DEV)
        net = vaw_amd.DistributedDataParallel(model, shard_optimizer=True)
        opt = vaw_amd.FusedAdamW(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
        assert opt.zero is not None
        opt.attach_ema_sharded(0.999)
        guard = vaw_amd.StepGuard(DEV)
        opt.attach_guard(guard)
        diff = _diffusion(base_args())
        g = torch.Generator().manual_seed(77)
        x, y = torch.randn(8, 4, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)
        t, noise = torch.randint(0, 1000, (8,), generator=g), torch.randn(8, 4, 8, 8, generator=g)
        x, y, t, noise = (v[4 * rank:4 * rank + 4].to(DEV) for v in (x, y, t, noise))
        snaps = []
        for step in range(3):                                  # clean, poisoned on rank 0 only, clean
            xs = x.clone()
            if step == 1 and rank == 0:
                xs[2, 1, 0, 3] = float("nan")
            terms = diff.training_losses(net, xs, None, t=t, model_kwargs={"y": y}, noise=noise)
            terms["loss"].mean().backward()
            opt.step()
            opt.zero_grad()
            opt.zero.wait_gathers()
            opt.consolidate()
            torch.cuda.synchronize()
            snaps.append(tuple(v.detach().cpu().numpy().copy() for v in (model._flat, opt.exp_avg, opt.exp_avg_sq, opt._ema_shard)))
        q.put((rank, snaps, guard.counters(), None))
        vaw_amd.dist_util.cleanup_dist()
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))


def test_sharded_optimizer_takes_the_same_decision_on_every_rank():
    """rank 0's batch is poisoned in step 2, rank 1's is clean: the all-reduced scalar gives both ranks the same verdict, the
    skipped step leaves each rank's weights, moment chunks and EMA shard as they were, and the gathered weights stay equal"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        rank, snaps, counters, err = q.get(timeout=300)
        assert err is None, err
        res[rank] = (snaps, counters)
    for p in procs:
        p.join(timeout=60)
    want = dict(ok=1, steps=3, applied=2, skipped_nonfinite=1, skipped_spike=0, in_a_row=0)
    for rank in (0, 1):
        snaps, counters = res[rank]
        assert counters == want, (rank, counters)
        for a, b in zip(snaps[0], snaps[1]):                  # the skipped step
            assert (a == b).all(), rank
        for a, b in zip(snaps[1], snaps[2]):
            assert not (a == b).all() and np.isfinite(b).all(), rank
    for a, b in zip(res[0][0], res[1][0]):
        assert (a[0] == b[0]).all()                           # the gathered weights: equal on both ranks after every step

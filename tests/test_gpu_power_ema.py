"""Post-hoc EMA on the device (csrc/ema.hip, vaw_amd.PowerEMA, vaw_amd.posthoc_ema, args.ema_sigma_rels): the profile update
bit for bit against the f32 tensor composition, the device's c_t against the host formula, the refusals, the float64 snapshot fold
bit for bit against numpy, the Trainer eager vs hipGraph vs resumed, and a reconstruction against a directly tracked profile.
Run on the MI355X box: pytest -m gpu."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import power_ema_cases as cases
from conftest import Pbar, base_args, perturb_, synth_loader

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd.ema import PowerEMA, lincomb_fold, posthoc_ema

DEV = "cuda"
WIDTHS = (0.05, 0.10, 0.02, 0.25)


def _updates(n, K, seed):
    """five updates of K profiles over n elements through the two kernels -> per update (p, c as float32, the K buffers after it)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    gamma = torch.tensor([cases.gamma_of(s) for s in WIDTHS[:K]], dtype=torch.float64, device=DEV)
    coef = torch.zeros(K, dtype=torch.float64, device=DEV)
    bufs = [torch.zeros(n, device=DEV) for _ in range(K)]
    out = []
    for _ in range(5):
        p = torch.randn(n, device=DEV, generator=g) * 3.0
        ops.ema_profiles_coef(step, gamma, coef)
        ops.ema_profiles_update(p, bufs, coef)
        out.append((p, coef.cpu().numpy().astype(np.float32), [b.clone() for b in bufs]))
    assert int(step.item()) == 5
    return out


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 16_388, 1_048_583])
def test_update_is_the_tensor_composition_bitwise(n, K):
    """n below, at and off the 16-byte group, below / above one 4096-element tile, and many tiles plus a partial one plus a tail"""
    run = _updates(n, K, seed=n + K)
    prev = [torch.zeros(n, device=DEV) for _ in range(K)]
    for t, (p, c, bufs) in enumerate(run, 1):
        for k in range(K):
            want = cases.composition(prev[k], p, c[k])
            assert torch.equal(bufs[k], want), (t, k, float(c[k]))
            if n <= 16_388:          # the same three roundings in numpy on the host
                e, q = prev[k].cpu().numpy(), p.cpu().numpy()
                assert np.array_equal(bufs[k].cpu().numpy(), q if c[k] == 1 else e + (q - e) * c[k])
        if t == 1:
            assert all(float(ck) == 1.0 for ck in c) and all(torch.equal(b, p) for b in bufs)          # update 1: an exact copy
        else:
            # (sigma_rel 0.02 has gamma = 47: c_2 = 1 - 2^-48 is 1 in float32, and the update a copy once more)
            assert all(0.0 < float(ck) <= 1.0 for ck in c) and all(float(ck) < 1.0 for ck in c[:2])
        prev = bufs
    again = _updates(n, K, seed=n + K)
    assert all(torch.equal(a, b) for (_, _, x), (_, _, y) in zip(run, again) for a, b in zip(x, y))


def test_first_update_overwrites_whatever_the_buffers_held():
    """c_1 == 1 takes p itself: e + (p - e) * 1 would round (and keep a NaN)"""
    n = 4099
    p = torch.randn(n, device=DEV)
    bufs = [torch.full((n,), float("nan"), device=DEV), torch.full((n,), 1e30, device=DEV)]
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    gamma = torch.tensor([cases.gamma_of(0.05), cases.gamma_of(0.10)], dtype=torch.float64, device=DEV)
    coef = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.ema_profiles_coef(step, gamma, coef)
    ops.ema_profiles_update(p, bufs, coef)
    assert torch.equal(bufs[0], p) and torch.equal(bufs[1], p)


def test_device_coefficients_match_the_host_formula():
    """c_t on the device against -expm1((gamma + 1) log1p(-1/t)) on the host, within 16 float64 ulp: two library calls at a few ulp
    each on either side, one product, and no amplification: expm1 is linear near 0, and where its argument is large c_t is close to
    1 and insensitive to it."""
    pe = PowerEMA(cases.walk_module(64).to(DEV), WIDTHS)
    for t in (1, 2, 3, 1000, 10 ** 6, 10 ** 7):
        sd = pe.state_dict()
        sd["step"] = t - 1
        pe.load_state_dict(sd)
        pe.update()
        assert pe.step == t
        got = pe.coefficients()
        for k, s in enumerate(WIDTHS):
            want = cases.coef(t, cases.gamma_of(s))
            ulp = abs(got[k] - want) / np.spacing(want)
            print(f"t {t} sigma_rel {s}: device {got[k]!r} host {want!r} ({ulp:.1f} ulp)")
            assert ulp <= 16 and abs(vaw_amd.power_ema_coefficient(t, pe.gammas[k]) - want) <= 4 * np.spacing(want)
        if t == 1:
            assert all(c == 1.0 for c in got)


def test_refusals_return_an_error_and_launch_nothing():
    n = 1024
    lib, s = vaw_amd.lib(), torch.cuda.current_stream().cuda_stream
    pool = torch.arange(4 * n + 64, dtype=torch.float32, device=DEV)
    before = pool.clone()
    p, e0, e1 = pool[:n], pool[n:2 * n], pool[2 * n:3 * n]
    coef = torch.full((4,), 0.5, dtype=torch.float64, device=DEV)
    ptr = lambda t: t.data_ptr()
    call = lambda p_, e0_, e1_, K, n_, c_=coef: lib.vaw_ema_profiles_update(ptr(p_), ptr(e0_), ptr(e1_), 0, 0, K, n_, ptr(c_), s)
    INVALID = vaw_amd._lib.CONSTANTS["ERR_INVALID"]
    assert call(pool[1:n + 1], e0, e1, 2, n) == INVALID                        # p offset by 4 bytes
    assert call(p, pool[n + 1:2 * n + 1], pool[2 * n + 4:3 * n + 4], 2, n) == INVALID          # e0 offset by 4 bytes
    assert call(p, p, e1, 2, n) == INVALID                                     # e0 aliases p
    assert call(p, e0, pool[n + 512:2 * n + 512], 2, n) == INVALID             # e1 overlaps e0
    assert call(p, e0, e1, 0, n) == INVALID and call(p, e0, e1, 5, n) == INVALID
    assert call(p, e0, e1, 2, 0) == INVALID and call(p, e0, e1, 2, -4) == INVALID
    assert lib.vaw_ema_profiles_update(ptr(p), ptr(e0), 0, 0, 0, 2, n, ptr(coef), s) == INVALID          # a needed pointer is NULL
    assert lib.vaw_ema_profiles_update(0, ptr(e0), ptr(e1), 0, 0, 2, n, ptr(coef), s) == INVALID
    assert lib.vaw_ema_profiles_update(ptr(p), ptr(e0), ptr(e1), 0, 0, 2, n, 0, s) == INVALID
    assert b"overlap" in lib.vaw_last_error_string() or b"NULL" in lib.vaw_last_error_string()
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.vaw_ema_profiles_coef(ptr(step), ptr(coef), ptr(coef), 0, s) == INVALID
    assert lib.vaw_ema_profiles_coef(ptr(step), ptr(coef), ptr(coef), 5, s) == INVALID
    assert lib.vaw_ema_profiles_coef(0, ptr(coef), ptr(coef), 2, s) == INVALID
    acc = torch.zeros(n, dtype=torch.float64, device=DEV)
    assert lib.vaw_lincomb_accum_f64(ptr(acc), ptr(p), 1.0, 0, s) == INVALID and lib.vaw_lincomb_accum_f64(0, ptr(p), 1.0, n, s) == INVALID
    assert lib.vaw_f64_to_f32(ptr(acc), ptr(acc), n, s) == INVALID and lib.vaw_f64_to_f32(ptr(acc), ptr(p), 0, s) == INVALID
    with pytest.raises(vaw_amd.VawError, match="overlaps"):
        ops.ema_profiles_update(p, [e0, e0], coef)
    with pytest.raises(vaw_amd.VawError):
        ops.ema_profiles_update(p, [e0, e1, pool[3 * n:4 * n], e0.clone(), e1.clone()], coef)
    torch.cuda.synchronize()
    assert torch.equal(pool, before) and int(step.item()) == 0 and float(acc.abs().sum()) == 0.0
    assert call(p, e0, e1, 2, n) == 0                                          # and the same operands, legal, are taken
    torch.cuda.synchronize()
    assert torch.equal(e0, before[n:2 * n] + (before[:n] - before[n:2 * n]) * 0.5)


def test_fold_is_numpys_float64_fold_bitwise():
    n, coefs = 1_048_583, (1.7, -0.9, 0.2)
    rng = np.random.default_rng(5)
    snaps = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32) for _ in coefs]
    acc = np.zeros(n, dtype=np.float64)
    for c, s in zip(coefs, snaps):
        acc += c * s.astype(np.float64)
    want = acc.astype(np.float32)
    tensors = [torch.from_numpy(s) for s in snaps]
    for chunk in (None, 333_333, 65_536, 1 << 20):          # whole tensors; odd chunks (element accesses); aligned chunks; one plus a tail
        got = lincomb_fold(iter(tensors), coefs, device=DEV, chunk=chunk)
        assert got.dtype == torch.float32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), chunk
    # the accumulator itself, before the rounding to f32
    a = torch.zeros(n, dtype=torch.float64, device=DEV)
    for c, t in zip(coefs, tensors):
        ops.lincomb_accum_f64(a, t.to(DEV), c)
    assert np.array_equal(a.cpu().numpy(), acc)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, graph, rels, **extra):
    if rels is not None:
        extra["ema_sigma_rels"] = rels
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, warmup_steps=3, cosine_decay=True,
                     total_steps=20, final_lr=1e-5, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph, amp=True,
                     logdir=str(tmp_path), model="DiT-tiny", mean_type="EPSILON", **extra)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="bf16").to(DEV)
    perturb_(model, 5)
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, synth_loader(8, 8, 8, 3, 10, latent=True), Pbar())
    return args, model, ema_model, opt, sched, tr


def _step(tr, s):
    torch.manual_seed(1000 + s)           # the device RNG stream of step s
    return float(tr.train_step(s))


def _forward(m):
    g = torch.Generator().manual_seed(3)
    x, t, y = torch.randn(4, 4, 8, 8, generator=g).to(DEV), torch.tensor([1.0, 250.0, 600.0, 999.0], device=DEV), torch.tensor([0, 3, 5, 9], device=DEV)
    m.eval()
    with torch.no_grad():
        return m(x, t, y=y)[0].float().clone()


RELS = (0.05, 0.10)


def test_trainer_tracks_profiles_eager_graph_and_resumed_bitwise(tmp_path):
    """6 steps of the tiny DiT.  With args.ema_sigma_rels every profile is, after every step, the composition applied to the
    parameters of that step; the model's own trajectory and the EMA copy are those of a run without the argument; the captured
    step (hip_graph=True) tracks the same bits; and a run resumed from the checkpoint of step 3 repeats steps 4-6."""
    args, model, ema_model, opt, sched, tr = _trainer(tmp_path, False, None)
    assert tr.power_ema is None
    plain = [_step(tr, s) for s in range(1, 7)], model._flat.clone(), ema_model._flat.clone()

    args, model, ema_model, opt, sched, tr = _trainer(tmp_path, False, RELS)
    pe = tr.power_ema
    assert isinstance(pe, PowerEMA) and pe.sigma_rels == list(RELS) and pe.step == 0
    prev, losses = [torch.zeros_like(f) for f in pe.flat], []
    for s in range(1, 7):
        losses.append(_step(tr, s))
        p, c = model._flat.clone(), pe.coefficients().astype(np.float32)
        assert pe.step == s and (s > 1 or all(ck == 1.0 for ck in c))
        for k in range(2):
            assert torch.equal(pe.flat[k], cases.composition(prev[k], p, c[k])), (s, k)
        prev = [f.clone() for f in pe.flat]
        if s == 3:
            path = vaw_amd.save_checkpoint(args, 3, model, opt, ema_model=ema_model, scheduler=sched, power_ema=pe)
    assert losses == plain[0] and torch.equal(model._flat, plain[1]) and torch.equal(ema_model._flat, plain[2])
    eager = prev
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[0], model._flat)

    # copy_to: the EMA copy then runs on the tracked profile
    before = _forward(ema_model)
    pe.copy_to(ema_model, 0.05)
    after = _forward(ema_model)
    loaded = copy.deepcopy(model)
    loaded.ensure_flat()
    loaded.load_state_dict({n: loaded._view_as_param(eager[0][o:o + k], q, loaded._flat_cl[n]).clone()
                            for (n, q) in loaded.named_parameters() for (o, k) in [loaded._flat_offsets[n]]})
    assert torch.equal(ema_model._flat, eager[0]) and not torch.equal(after, before) and torch.equal(after, _forward(loaded))

    args, model_g, ema_g, opt_g, sched_g, tr_g = _trainer(tmp_path, True, RELS)
    assert [_step(tr_g, s) for s in range(1, 7)] == losses and tr_g._graph is not None
    assert tr_g.power_ema.step == 6 and all(torch.equal(a, b) for a, b in zip(tr_g.power_ema.flat, eager))
    assert torch.equal(model_g._flat, plain[1]) and torch.equal(ema_g._flat, plain[2])

    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"model", "optimizer", "step", "ema_model", "scheduler", "power_ema"} and ck["power_ema"]["step"] == 3
    args, model_r, ema_r, opt_r, sched_r, tr_r = _trainer(tmp_path, False, RELS)
    with torch.no_grad():                      # nothing survives from the constructor
        model_r.flat_params().add_(1.0)
    vaw_amd.load_checkpoint(path, model=model_r, optimizer=opt_r, ema_model=ema_r, scheduler=sched_r, power_ema=tr_r.power_ema)
    assert tr_r.power_ema.step == 3
    assert [_step(tr_r, s) for s in range(4, 7)] == losses[3:]
    for k in range(2):
        for name, (o, n) in model_r._flat_offsets.items():           # (the flat buffers also hold alignment gaps: compare entries)
            assert torch.equal(tr_r.power_ema.flat[k][o:o + n], eager[k][o:o + n]), (k, name)


def test_trainer_snapshots_auto_graph_and_rebuilt_buffer(tmp_path):
    args, model, ema_model, opt, sched, tr = _trainer(tmp_path, "auto", RELS, ema_snapshot_every=2, ema_snapshot_dir=os.path.join(tmp_path, "snaps"))
    for s in range(1, 5):
        _step(tr, s)
    files = sorted(os.listdir(args.ema_snapshot_dir))
    assert files == ["power_ema_00000002.pt", "power_ema_00000004.pt"]
    snap = torch.load(os.path.join(args.ema_snapshot_dir, files[-1]), weights_only=True)
    assert snap["step"] == 4 and all(torch.equal(a, b.cpu()) for a, b in zip(snap["flat"], tr.power_ema.flat))
    with pytest.raises(ValueError, match="ema_snapshot_dir"):
        _trainer(tmp_path, False, RELS, ema_snapshot_every=2)
    model._build_flat()                        # the buffer the averages follow is gone: refuse, as FusedAdamW.step does
    with pytest.raises(RuntimeError, match="rebuilt"):
        tr.power_ema.update()


# ---- reconstruction ---------------------------------------------------------------------------------------------------------------
def test_posthoc_ema_reconstructs_a_directly_tracked_profile(tmp_path):
    """The CPU test's random walk at width 1024, stepped as a FlatModule on the device and tracked in f32: the default two widths
    with a snapshot every 256 steps, and 0.075 directly.  The reconstruction of 0.075 at T from the snapshots is within 2e-3 of
    the direct profile, in units of max |direct - theta_T|; the tracked widths themselves come back within 1e-5 (f32 buffers)."""
    T, W = 4096, 1024
    theta = torch.from_numpy(cases.random_walk(T, W)).float().to(DEV)
    m = cases.walk_module(W).to(DEV)
    m.ensure_flat()
    pe, direct = PowerEMA(m), PowerEMA(m, (0.075,))
    snaps = []
    with torch.no_grad():
        for t in range(1, T + 1):
            m._flat[:W].copy_(theta[t - 1])
            pe.update()
            direct.update()
            if t % 256 == 0:
                snaps.append(pe.snapshot() if t % 512 else pe.save_snapshot(os.path.join(tmp_path, f"s{t}.pt")))          # dicts and paths
    assert len(snaps) == 16 and pe.step == T
    scale = float((direct.flat[0] - m._flat).abs().max())
    into = cases.walk_module(W).to(DEV)
    got, coefs = posthoc_ema(snaps, 0.075, into=into, return_coefficients=True)
    err = float((got - direct.flat[0]).abs().max()) / scale
    print(f"sigma_rel 0.075 at T: relative error {err:.3g} (scale {scale:.3g})")
    assert got.data_ptr() == into._flat.data_ptr() and err <= 2e-3
    steps, rels = [t for t in range(256, T + 1, 256) for _ in RELS], [s for _ in range(16) for s in RELS]
    assert np.array_equal(coefs, vaw_amd.posthoc_coefficients(steps, rels, T, 0.075)) and posthoc_ema.last_coefficients is coefs
    for s in RELS:
        back = posthoc_ema(snaps, s, device=DEV)
        err = float((back - pe.flat[RELS.index(s)]).abs().max()) / scale
        print(f"sigma_rel {s} at T: relative error {err:.3g}")
        assert err <= 1e-5
    # an earlier time: only the snapshots up to it take part, and the tracked profile there is the stored one
    early = posthoc_ema(snaps, 0.05, step=1024, device=DEV)
    stored = snaps[3] if isinstance(snaps[3], dict) else torch.load(snaps[3], weights_only=True)
    assert stored["step"] == 1024 and float((early.cpu() - stored["flat"][0]).abs().max()) / scale <= 1e-5
    assert all(c == 0.0 for c, t in zip(posthoc_ema.last_coefficients, steps) if t > 1024)

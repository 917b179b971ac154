"""The device-resident loss-second-moment sampler (vaw_resampler_update / vaw_resampler_draw, DeviceLossSecondMomentResampler,
args.schedule_sampler = "loss-second-moment-device") against the host LossSecondMomentResampler: the history bit for bit, p
within a few f64 roundings, the draws exactly what numpy's search gives on the device's own p, numpy-stream parity with the
host sampler's sample(), the Trainer eager vs hipGraph vs resumed from a checkpoint, and two ranks.  Run on the MI355X box:
pytest -m gpu."""
import copy
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

from conftest import REPO, Pbar, base_args, perturb_, synth_loader

pytestmark = pytest.mark.gpu

import vaw_amd

DEV = "cuda"
SHAPES = [(7, 3, 5), (7, 3, 1), (1, 10, 4), (1000, 10, 256), (1000, 10, 257), (1000, 10, 4099)]      # (T, H, n)
# p against the host's weights() / weights().sum(): largest relative difference over SHAPES measured on an MI355X 8.525e-16 (at
# (1000, 10, 4099); per shape in test_weights_match_the_host_sampler).  The bound is 16 x that, and may never exceed 1e-12
P_REL_MEASURED = 8.525e-16
P_REL_BOUND = 16 * P_REL_MEASURED
assert P_REL_BOUND <= 1e-12


def _diff(T, **args):
    return SimpleNamespace(num_timesteps=T, args=SimpleNamespace(**args))


def _pair(T, H, uniform_prob=0.001):
    d = _diff(T)
    return vaw_amd.LossSecondMomentResampler(d, H, uniform_prob), vaw_amd.DeviceLossSecondMomentResampler(d, DEV, H, uniform_prob)


def _losses(rng, ts, zero_t=None):
    """f32 losses spanning 1e-6 .. 1e3; timestep zero_t only ever sees 0.0"""
    v = (10.0 ** rng.uniform(-6, 3, size=len(ts))).astype(np.float32)
    if zero_t is not None:
        v[np.asarray(ts) == zero_t] = 0.0
    return v


def _feed(host, dev, ts, losses):
    """the same pairs to both; the host only gets the ones in range (the device must skip the others itself)"""
    ts, losses = np.asarray(ts, dtype=np.int64), np.asarray(losses, dtype=np.float32)
    ok = (ts >= 0) & (ts < host.diffusion.num_timesteps)
    host.update_with_all_losses(ts[ok].tolist(), losses[ok].tolist())
    dev.update_with_local_losses(torch.from_numpy(ts).to(DEV), torch.from_numpy(losses).to(DEV))


def _same_history(host, dev):
    ring, seen = dev.ring.cpu(), dev.seen.cpu()
    assert ring.dtype == torch.float64 and seen.dtype == torch.int64
    return torch.equal(ring, torch.from_numpy(host._ring)) and torch.equal(seen, torch.from_numpy(host._seen))


_WARM = {}


def _warm_pair(T, H, n):
    """a host / device pair with a full, non-uniform history, built once per shape and never modified afterwards: H batches
    that visit every timestep, then three random batches of n (timestep T // 2 has an all-zero history when T > 1)"""
    key = (T, H, n)
    if key not in _WARM:
        rng = np.random.RandomState(1000 * T + 10 * H + n)
        host, dev = _pair(T, H)
        zero_t = T // 2 if T > 1 else None
        for _ in range(H):
            ts = rng.permutation(T)
            _feed(host, dev, ts, _losses(rng, ts, zero_t))
        for _ in range(3):
            ts = rng.randint(0, T, size=n)
            _feed(host, dev, ts, _losses(rng, ts, zero_t))
        assert host._warmed_up() and _same_history(host, dev)
        if zero_t is not None:
            assert not host._ring[zero_t].any()
        _WARM[key] = (host, dev)
    return _WARM[key]


# ---- update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,n", SHAPES)
def test_update_matches_the_host_ring_bitwise(T, H, n):
    rng = np.random.RandomState(T + H + n)
    host, dev = _pair(T, H)
    for call in range(4):
        ts = rng.randint(0, T, size=n)
        if (T, H, n) == (7, 3, 5) and call % 2 == 0:
            ts[:] = 4                                   # one timestep five times in a call: the 3-slot ring wraps inside the batch
        _feed(host, dev, ts, _losses(rng, ts))
        assert _same_history(host, dev), call
    assert dev.invalid_count() == 0 and int(dev.seen.sum()) == 4 * n


def test_update_skips_and_counts_timesteps_out_of_range():
    host, dev = _pair(7, 3)
    _feed(host, dev, [3, -1, 2, 7, 3, 0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert dev.invalid_count() == 2
    assert _same_history(host, dev) and int(dev.seen.sum()) == 4
    _feed(host, dev, [6, 6], [0.5, 0.25])
    assert dev.invalid_count() == 2 and _same_history(host, dev)
    _feed(host, dev, [1 << 40, -(1 << 40), 5], [1.0, 1.0, 7.0])          # far outside int32 too
    assert dev.invalid_count() == 4 and _same_history(host, dev)


# ---- warm-up edge ---------------------------------------------------------------------------------------------------------------
def test_warm_up_edge():
    T, H = 7, 3
    rng = np.random.RandomState(5)
    host, dev = _pair(T, H)
    for k in range(H):                                  # every timestep gets H entries, the last one only H - 1
        ts = np.arange(T if k < H - 1 else T - 1)
        _feed(host, dev, ts, _losses(rng, ts))
    assert not host._warmed_up()
    idx, w = dev.sample(64)
    p = dev.weights()
    assert np.array_equal(p, np.full(T, 1.0 / T))
    assert torch.equal(w.cpu(), torch.ones(64)) and int(idx.min()) >= 0 and int(idx.max()) < T
    _feed(host, dev, [T - 1], [0.125])                  # the one update that completes the last timestep
    assert host._warmed_up()
    p = dev.weights()
    assert not np.array_equal(p, np.full(T, 1.0 / T))
    ref = host.weights() / host.weights().sum()
    rel = float(np.max(np.abs(p - ref) / ref))
    print(f"[resample warm-up edge] p vs host: max rel {rel:.3e}")
    assert rel <= P_REL_BOUND
    _, w = dev.sample(64)
    assert not torch.equal(w.cpu(), torch.ones(64))


# ---- weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,n", SHAPES)
def test_weights_match_the_host_sampler(T, H, n):
    """Oracle: the host LossSecondMomentResampler.weights() on the same (bitwise equal) history, normalised.  numpy sums pairwise,
    the kernel in the fixed orders of include/vaw_hip.h, so the two differ by a few f64 roundings.  Largest relative
    difference measured on an MI355X, per (T, H, n): (7, 3, 5) 0, (7, 3, 1) 2.631e-16, (1, 10, 4) 0, (1000, 10, 256) 4.714e-16,
    (1000, 10, 257) 4.766e-16, (1000, 10, 4099) 8.525e-16; the warm-up edge test's history 2.827e-16."""
    host, dev = _warm_pair(T, H, n)
    p = dev.weights()
    ref = host.weights() / host.weights().sum()
    assert p.dtype == np.float64 and p.shape == (T,) and np.all(p > 0)
    rel = float(np.max(np.abs(p - ref) / ref))
    print(f"[resample weights T {T} H {H} n {n}] p vs host: max rel {rel:.3e}, sum p - 1 = {p.sum() - 1:.3e}")
    assert rel <= P_REL_BOUND
    if T > 1:
        assert p.std() > 0 and p[T // 2] == p.min()      # the all-zero timestep keeps only the uniform floor
        assert p[T // 2] == pytest.approx(dev.uniform_prob / T, rel=1e-12)


# ---- draw -------------------------------------------------------------------------------------------------------------------------
def _far_from(c, u, eps=1e-9):
    """mask of the uniforms that are not within eps of an entry of the CDF c"""
    k = np.searchsorted(c, u)
    lo, hi = c[np.clip(k - 1, 0, len(c) - 1)], c[np.clip(k, 0, len(c) - 1)]
    return (np.abs(u - lo) > eps) & (np.abs(u - hi) > eps)


@pytest.mark.parametrize("T,B", [(7, 1), (7, 64), (1000, 4096), (1000, 4097)])
def test_draw_is_numpys_search_on_the_devices_own_p(T, B):
    host, dev = _warm_pair(T, 3 if T == 7 else 10, 5 if T == 7 else 257)
    u = np.random.RandomState(B).random_sample(B)
    idx, w = dev._draw(torch.from_numpy(u).to(DEV))
    p = dev._p.cpu().numpy()
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert idx.dtype == np.int64 and w.dtype == np.float32 and idx.shape == w.shape == (B,)
    c = np.cumsum(p)
    c /= c[-1]
    keep = _far_from(c, u)
    assert (~keep).sum() < 0.01 * B
    assert np.array_equal(idx[keep], np.searchsorted(c, u[keep], side="right"))
    assert idx.min() >= 0 and idx.max() < T
    assert np.array_equal(w, (1.0 / (T * p[idx])).astype(np.float32))              # every draw: bitwise, on the index it returned
    if B >= 64 and T > 1:
        assert len(set(idx.tolist())) > 1
    # the ends of [0, 1)
    ends = np.array([0.0, np.nextafter(1.0, 0.0)])
    ie, we = dev._draw(torch.from_numpy(ends).to(DEV))
    ie = ie.cpu().numpy()
    assert ie[0] == np.searchsorted(c, 0.0, side="right") == 0 and 0 <= ie[1] < T
    assert np.array_equal(we.cpu().numpy(), (1.0 / (T * p[ie])).astype(np.float32))


def test_draw_at_the_largest_T_and_refusal_just_above():
    """T = VAW_RESAMPLER_MAX_T fills the draw's 64 KiB of LDS; one more is refused with the library's message."""
    T = vaw_amd._lib.RESAMPLER_MAX_T
    dev = vaw_amd.DeviceLossSecondMomentResampler(_diff(T), DEV, 2)
    rng = np.random.RandomState(0)
    ring = (10.0 ** rng.uniform(-3, 1, size=(T, 2)))
    dev.load_state_dict({"ring": torch.from_numpy(ring), "seen": torch.full((T,), 2, dtype=torch.int64)})
    u = rng.random_sample(257)
    idx, w = dev._draw(torch.from_numpy(u).to(DEV))
    p = dev._p.cpu().numpy()
    host = dev.to_host()
    ref = host.weights() / host.weights().sum()
    rel = float(np.max(np.abs(p - ref) / ref))
    print(f"[resample weights T {T} H 2] p vs host: max rel {rel:.3e}")
    assert rel <= P_REL_BOUND
    c = np.cumsum(p)
    c /= c[-1]
    keep = _far_from(c, u)
    assert (~keep).sum() < 0.01 * len(u)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx[keep], np.searchsorted(c, u[keep], side="right"))
    assert np.array_equal(w.cpu().numpy(), (1.0 / (T * p[idx])).astype(np.float32))
    big = vaw_amd.DeviceLossSecondMomentResampler(_diff(T + 1), DEV, 2)
    with pytest.raises(vaw_amd.VawError, match=str(T + 1)):
        big.sample(4)
    big.update_with_all_losses(torch.tensor([T], device=DEV), torch.tensor([1.0], device=DEV))       # the update has no such bound
    assert int(big.seen[T]) == 1


# ---- numpy-stream parity with the host sampler --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(7, 64), (1000, 4096)])
def test_sample_reproduces_the_host_sampler_on_numpys_stream(T, B):
    host, dev0 = _warm_pair(T, 3 if T == 7 else 10, 5 if T == 7 else 257)
    dev = vaw_amd.DeviceLossSecondMomentResampler.from_host(host, DEV)
    assert torch.equal(dev.ring, dev0.ring) and torch.equal(dev.seen, dev0.seen) and not dev.cpu_rng
    dev.cpu_rng = True                                   # what a diffusion built with args.cpu_rng gives
    assert vaw_amd.DeviceLossSecondMomentResampler(_diff(T, cpu_rng=True), DEV).cpu_rng
    np.random.seed(77)
    hi, hw = host.sample(B, "cpu")
    np.random.seed(77)
    di, dw = dev.sample(B, DEV)
    np.random.seed(77)
    u = np.random.random_sample(B)                       # the uniforms both consumed
    w = host.weights()
    c = np.cumsum(w / np.sum(w))
    c /= c[-1]
    keep = _far_from(c, u)
    assert (~keep).sum() < 0.01 * B
    assert np.array_equal(hi.numpy()[keep], np.searchsorted(c, u[keep], side="right"))        # (the reference consumed u this way)
    assert torch.equal(di.cpu()[keep], hi[keep])
    assert hw.dtype == dw.dtype == torch.float32 and torch.equal(dw.cpu()[keep], hw[keep])
    back = dev.to_host()
    assert np.array_equal(back._ring, host._ring) and np.array_equal(back._seen, host._seen)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------------
def _history(T, H):
    rng = np.random.RandomState(11)
    return {"ring": torch.from_numpy(10.0 ** rng.uniform(-2, 0.5, size=(T, H))), "seen": torch.from_numpy(rng.randint(H, 5 * H, size=T))}


def _trainer(tmp_path, graph):
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, warmup_steps=3, cosine_decay=True,
                     total_steps=20, final_lr=1e-5, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph, amp=True,
                     schedule_sampler="loss-second-moment-device", logdir=str(tmp_path), model="DiT-tiny", mean_type="EPSILON")
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
    assert isinstance(tr.schedule_sampler, vaw_amd.DeviceLossSecondMomentResampler)
    return args, model, ema_model, opt, sched, tr


def _steps(tr, first, n):
    out = []
    for s in range(first, first + n):
        torch.manual_seed(1000 + s)           # the device RNG stream of step s (latent sampling, uniforms of the sampler, noise)
        out.append(float(tr.train_step(s)))
    return out


def test_trainer_eager_vs_hip_graph_vs_resumed_is_bitwise(tmp_path):
    """6 steps of the tiny DiT with the device sampler, warm from step 1 (a full history is loaded first, so p is not uniform):
    eager == hip_graph=True (draw, uniforms and update captured with the step) in every loss, the final parameters and the
    sampler's history, bit for bit; and a fresh eager run resumed from the checkpoint written after step 3 repeats steps 4-6."""
    hist = _history(1000, 10)
    runs = {}
    for graph in (False, True):
        args, model, ema_model, opt, sched, tr = _trainer(tmp_path, graph)
        tr.schedule_sampler.load_state_dict(hist)
        losses = _steps(tr, 1, 3)
        if not graph:
            path = vaw_amd.save_checkpoint(args, 3, model, opt, ema_model=ema_model, scheduler=sched, schedule_sampler=tr.schedule_sampler)
        losses += _steps(tr, 4, 3)
        assert (tr._graph is not None) == graph
        s = tr.schedule_sampler
        runs[graph] = (losses, model._flat.clone(), ema_model._flat.clone(), s.ring.clone(), s.seen.clone())
        assert s.invalid_count() == 0
    (le, pe, ee, re_, se), (lg, pg, eg, rg, sg) = runs[False], runs[True]
    assert all(np.isfinite(le)) and le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(ee, eg)
    assert torch.equal(re_, rg) and torch.equal(se, sg)
    assert int(se.sum()) == int(hist["seen"].sum()) + 6 * 8 and not torch.equal(re_.cpu(), hist["ring"])
    w = tr.schedule_sampler.weights()
    assert w.std() > 0 and abs(w.sum() - 1.0) < 1e-12

    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"model", "optimizer", "step", "ema_model", "scheduler", "schedule_sampler"}
    args, model, ema_model, opt, sched, tr = _trainer(tmp_path, False)
    with torch.no_grad():                      # nothing survives from the constructor
        model.flat_params().add_(1.0)
    assert int(tr.schedule_sampler.seen.sum()) == 0
    vaw_amd.load_checkpoint(path, model=model, optimizer=opt, ema_model=ema_model, scheduler=sched, schedule_sampler=tr.schedule_sampler)
    assert _steps(tr, 4, 3) == le[3:]
    s = tr.schedule_sampler
    assert torch.equal(s.ring, re_) and torch.equal(s.seen, se)
    for m, flat in ((model, pe), (ema_model, ee)):           # (the flat buffers also hold alignment gaps: compare entries)
        for name, (o, n) in m._flat_offsets.items():
            assert torch.equal(m._flat[o:o + n], flat[o:o + n]), name


def test_trainer_hip_graph_auto_accepts_the_device_sampler():
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, hip_graph="auto", defer_loss_sync=True,
                     schedule_sampler="loss-second-moment-device")
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.0,
                        num_classes=10, learn_sigma=False, compute_dtype="bf16").to(DEV)
    opt = vaw_amd.FusedAdamW(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, None, opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: 1.0), diff,
                         synth_loader(8, 8, 8, 3, 10, latent=True), Pbar())
    assert tr._use_graph and tr._graph_auto and tr._device_sampler
    args.schedule_sampler = "loss-second-moment"
    with pytest.raises(ValueError, match="hip_graph"):
        vaw_amd.Trainer(args, torch.device(DEV), model, None, opt, None, diff, [], Pbar())


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------
def _rank_stream():
    """three updates of two ranks, five pairs each, on a 13-step process with 3-slot rings (repeats and wraps inside a call)"""
    rng = np.random.RandomState(21)
    ts = rng.randint(0, 13, size=(3, 2, 5))
    ts[1, :, :3] = 9
    return ts, (10.0 ** rng.uniform(-6, 3, size=(3, 2, 5))).astype(np.float32)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, REPO)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import vaw_amd
        vaw_amd.dist_util.setup_dist(backend="gloo", device_index=0)
        dev = torch.device("cuda", 0)
        s = vaw_amd.DeviceLossSecondMomentResampler(_diff(13), dev, 3)
        ts, losses = _rank_stream()
        for k in range(3):
            s.update_with_local_losses(torch.from_numpy(ts[k, rank]).to(dev), torch.from_numpy(losses[k, rank]).to(dev))
        q.put((rank, s.ring.cpu().numpy(), s.seen.cpu().numpy(), s.invalid_count(), None))      # by value: the worker exits first
        vaw_amd.dist_util.cleanup_dist()
    except Exception:
        q.put((rank, None, None, None, traceback.format_exc()))


def test_two_ranks_hold_the_single_rank_history():
    ts, losses = _rank_stream()
    host, one = _pair(13, 3)
    for k in range(3):
        _feed(host, one, ts[k].reshape(-1), losses[k].reshape(-1))            # rank-major concatenation
    assert _same_history(host, one)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        rank, ring, seen, bad, err = q.get(timeout=300)
        assert err is None, err
        res[rank] = (torch.from_numpy(ring), torch.from_numpy(seen), bad)
    for p in procs:
        p.join(timeout=60)
    for rank in (0, 1):
        ring, seen, bad = res[rank]
        assert ring.dtype == torch.float64 and seen.dtype == torch.int64 and bad == 0
        assert torch.equal(ring, one.ring.cpu()) and torch.equal(seen, one.seen.cpu()), rank

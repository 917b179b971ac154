"""Activation recomputation of the HIP DiT (DiT(activation_checkpointing=True)): the recomputed records are the first forward's
bit for bit, the model and its gradients are the ones the resident layout gives (and the reference's fixtures), the
workspace is what vaw_dit_ws_plan says, hooks / accumulation / Trainer / hipGraph keep working.  Tiny shapes: image 8,
patch 2 (T = 16), hidden 64, 2 heads, batch 4 (M = 64 rows: the bf16 deferred weight-gradient mode is live), depth 3 and 4
(4: the early adaLN bucket of the gradient hooks).  Run on the MI355X box: pytest -m gpu."""
import copy
import random

import numpy as np
import pytest
import torch

from conftest import Pbar, assert_fingerprints, base_args, load_json, load_pt, perturb_, synth_loader

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops

DEV = "cuda"
KW = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, num_heads=2, class_dropout_prob=0.0, num_classes=10,
          learn_sigma=False)
FWD_KEYS = ("xm", "qkv", "ao", "lse", "y1", "xm2", "hpre", "a", "y2", "mean1", "rstd1", "mean2", "rstd2")
_INPUTS = {}


def _inputs():
    if not _INPUTS:
        g = torch.Generator().manual_seed(1)
        _INPUTS.update(x=torch.randn(4, 4, 8, 8, generator=g).to(DEV), t=(torch.rand(4, generator=g) * 999).to(DEV),
                       y=torch.randint(0, 10, (4,), generator=g).to(DEV), gout=torch.randn(4, 4, 8, 8, generator=g).to(DEV))
    return _INPUTS


def _make(depth, dtype, ckpt, defer=True):
    torch.manual_seed(5)
    m = vaw_amd.DiT(depth=depth, compute_dtype=dtype, activation_checkpointing=ckpt, **KW)
    perturb_(m, 6)                         # off the adaLN-Zero init: every gate is live
    m = m.to(DEV).train()
    m.defer_wgrad = defer
    m.ensure_flat()
    return m


def _step(m, need_dx=True):
    """forward + backward on the shared inputs: (out, dx, flat gradients)"""
    i = _inputs()
    xr = i["x"].clone().requires_grad_(need_dx)
    out, _ = m(xr, i["t"], i["y"])
    (out * i["gout"]).sum().backward()
    return out.detach(), (xr.grad.clone() if need_dx else None), m.flat_grads().clone()


_RUNS = {}


def _run(depth, dtype, ckpt, defer=True):
    """one step of a fresh model, computed once per configuration and shared (never modified) by the tests below"""
    key = (depth, dtype, ckpt, defer)
    if key not in _RUNS:
        m = _make(depth, dtype, ckpt, defer)
        _RUNS[key] = (m,) + _step(m)
    return _RUNS[key]


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_recompute_is_exact(dtype, depth):
    """The shared record after the forward's last block == the record right after block L-1 was recomputed in backward, every
    buffer, bit for bit; and every block's recomputed record == that block's record of a model that keeps them all."""
    m = _make(depth, dtype, True)
    i = _inputs()
    out, _ = m(i["x"], i["t"], i["y"])
    ws = m._ws_cur
    assert ws.ckpt and len({id(b) for b in ws.blk}) == 1
    first = {k: ws.blk[0][k].clone() for k in FWD_KEYS}
    first["xres_mid"] = ws.xres[1].clone()
    rows = [ws.xres[2 * l].clone() for l in range(depth + 1)]
    seen = {}

    def grab(l, rec):
        seen[l] = {k: rec[k].clone() for k in FWD_KEYS}
        seen[l]["xres_mid"], seen[l]["xout"] = ws.xres[2 * l + 1].clone(), ws.xscr.clone()

    m._ckpt_debug_hook = grab
    (out * i["gout"]).sum().backward()
    m._ckpt_debug_hook = None
    assert sorted(seen) == list(range(depth))
    for k, v in first.items():
        assert v.dtype == seen[depth - 1][k].dtype and torch.equal(v, seen[depth - 1][k]), k
    ref = _run(depth, dtype, False)[0]._ws_cur
    assert not ref.ckpt and len({id(b) for b in ref.blk}) == depth
    for l in range(depth):
        for k in FWD_KEYS:
            assert torch.equal(seen[l][k], ref.blk[l][k]), (l, k)
        assert torch.equal(seen[l]["xres_mid"], ref.xres[2 * l + 1]), l
        assert torch.equal(seen[l]["xout"], ref.xres[2 * l + 2]), l         # fc2's residual output went to the scratch row ...
        assert torch.equal(ws.xres[2 * l], rows[l]) and torch.equal(rows[l], ref.xres[2 * l]), l      # ... the input rows survived
    assert torch.equal(ws.xres[2 * depth], rows[depth])


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_same_model_forward_output_is_bitwise(dtype, depth):
    on, off = _run(depth, dtype, True), _run(depth, dtype, False)
    assert float(off[1].abs().max()) > 0
    assert torch.equal(on[1], off[1])


@pytest.mark.parametrize("tag", ["p2", "p4"])
def test_dit_tiny_fp32_checkpointed_matches_reference_golden(tag):
    """test_gpu_dit.py::test_dit_tiny_fp32_matches_reference_golden with the flag on: same fixture, same tolerances, and the
    gradient-accumulation bounds of that test."""
    g = load_pt("dit_tiny.pt")
    torch.manual_seed(11)
    m = vaw_amd.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="fp32",
                    activation_checkpointing=True, **g[f"{tag}/kw"])
    m = m.to(DEV).train()
    x, t, y, gout = (g[f"{tag}/{k}"].to(DEV) for k in ("x", "t", "y", "gout"))
    perturb_(m, 99)
    assert_fingerprints({k: v.cpu() for k, v in m.state_dict().items()}, g[f"{tag}/sd"], 1e-6, 1e-9, "perturbed")
    xr = x.clone().requires_grad_(True)
    out, _ = m(xr, t, y)
    (out * gout).sum().backward()
    assert m._ws_cur.ckpt
    torch.testing.assert_close(out.detach().cpu(), g[f"{tag}/out"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(xr.grad.cpu(), g[f"{tag}/gx"], rtol=1e-4, atol=2e-5)
    grads = {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}
    assert_fingerprints(grads, g[f"{tag}/grads"], 1e-4, 2e-5, "parameter gradients")
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


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_per_layer_weight_gradients_on_and_off_are_bitwise(dtype, depth):
    """defer_wgrad=False (and f32 always): the same launch per Linear layer in both modes, and the unfused LayerNorm-backward /
    gate-backward pair the recomputing backward uses is bitwise the fused pass -- every gradient and dx is identical."""
    on, off = _run(depth, dtype, True, defer=False), _run(depth, dtype, False, defer=False)
    assert not on[0]._ws_cur.defer and not off[0]._ws_cur.defer
    assert float(off[3].abs().max()) > 0 and float(off[2].abs().max()) > 0
    assert torch.equal(on[2], off[2])
    assert torch.equal(on[3], off[3])


def _worst_rel(m, a, b):
    """worst over the parameter tensors of max |a - b| / max |b|"""
    worst = 0.0
    for name, (o, n) in m._flat_offsets.items():
        if o + n <= m._flat_n_train and float(b[o:o + n].abs().max()) > 0:
            worst = max(worst, float((a[o:o + n] - b[o:o + n]).abs().max() / b[o:o + n].abs().max()))
    return worst


@pytest.mark.parametrize("depth", [3, 4])
def test_bf16_deferred_weight_gradients_on_vs_off(depth):
    """bf16 with deferred weight gradients: the flag groups the weight-gradient problems per block instead of all blocks at once.
    Worst relative difference over the parameter tensors (max |a - b| / max |b| per tensor) and of dx: on vs off, and each of
    on / off vs an f32 run of the same model.  Measured on an MI355X:
        depth 3: on vs off 0 (bitwise)   on vs f32 7.386e-03   off vs f32 7.386e-03
        depth 4: on vs off 0 (bitwise)   on vs f32 9.352e-03   off vs f32 9.352e-03
    A problem of the grouped launch is computed the same way whatever else is in its group, so on vs off is bitwise here too:
    that is what is asserted (it implies on vs off <= off vs f32)."""
    on, off, f32 = _run(depth, "bf16", True), _run(depth, "bf16", False), _run(depth, "fp32", False)
    assert on[0]._ws_cur.defer and off[0]._ws_cur.defer and on[0]._ws_cur.plan.own_dy
    m = on[0]
    rel_dx = lambda a, b: float((a - b).abs().max() / b.abs().max())
    on_off = max(_worst_rel(m, on[3], off[3]), rel_dx(on[2], off[2]))
    on_f32 = max(_worst_rel(m, on[3], f32[3]), rel_dx(on[2], f32[2]))
    off_f32 = max(_worst_rel(m, off[3], f32[3]), rel_dx(off[2], f32[2]))
    print(f"[ckpt bf16 deferred, depth {depth}] on vs off {on_off:.3e}   on vs f32 {on_f32:.3e}   off vs f32 {off_f32:.3e}")
    assert 0 < off_f32 < 3e-2          # (bf16: 8 significant bits through ~10 roundings, as test_dit_tiny_bf16_close_to_reference)
    assert on_off <= off_f32
    assert torch.equal(on[3], off[3]) and torch.equal(on[2], off[2])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gradient_accumulation_with_the_flag_on(dtype):
    """two backward passes without zeroing = 2 x one pass (bounds of test_gpu_dit.py's accumulation check)"""
    m, _, _, g1 = _run(4, dtype, True)
    m2 = _make(4, dtype, True)
    _step(m2)
    _, _, g2 = _step(m2)
    torch.testing.assert_close(g2, 2 * g1, rtol=1e-5, atol=1e-6)
    m2.zero_grad_flat()
    _, _, g3 = _step(m2)
    torch.testing.assert_close(g3, g1, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gradient_hooks_order_and_ranges_are_final(dtype, depth):
    """Stages arrive as depth+1, depth, ..., 1 with "ada_hi" right after the first block of the upper half (depth >= 4), then 0;
    when a stage is reported, its ranges of the flat gradient buffer already hold their final values."""
    m = _make(depth, dtype, True)
    bounds = m.grad_stage_bounds()
    snaps = []

    def hook(stage):
        rng = bounds[stage]
        snaps.append((stage, [(lo, hi, m.flat_grads()[lo:hi].clone()) for lo, hi in (rng if isinstance(rng, list) else [rng])]))

    m.grad_ready_hook = hook
    _, _, final = _step(m)
    m.grad_ready_hook = None
    want = list(range(depth + 1, 0, -1)) + [0]
    if depth >= 4:
        assert m._ada_split_block() == depth // 2
        want.insert(want.index(depth // 2 + 1) + 1, "ada_hi")
    else:
        assert "ada_hi" not in bounds
    assert [s for s, _ in snaps] == want
    cover = torch.zeros(m._flat_n_train, dtype=torch.int32)
    for stage, parts in snaps:
        for lo, hi, v in parts:
            cover[lo:hi] += 1
            assert torch.equal(v, final[lo:hi]), (stage, lo, hi)
    assert int(cover.min()) == 1 and int(cover.max()) == 1
    # the head's and the blocks' gradients are those of a run without a listener, bit for bit (the same launches; only the packed
    # adaLN weight gradient is cut differently for the early bucket)
    plain = _run(depth, dtype, True)[3]
    for stage in range(1, depth + 2):
        lo, hi = bounds[stage]
        assert torch.equal(final[lo:hi], plain[lo:hi]), stage


def _ws_tensors(ws):
    """every tensor the workspace holds, once: its attributes, lists, records and partial-sum sets -- not the descriptor tables
    of the cached launch groups, the caller's labels or the plan"""
    found = {}

    def walk(o):
        if isinstance(o, torch.Tensor):
            found[o.data_ptr()] = o
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, ops.ColsumPartial):
            walk(o.buf)

    for name, v in vars(ws).items():
        if name not in ("wgrad_groups", "bias_groups", "y", "_bufs", "plan"):
            walk(v)
    return list(found.values())


def _plan_of(m, B, ckpt):
    from vaw_amd import _lib as L
    return ops.dit_ws_plan(L.BF16 if m.compute_dtype == "bf16" else L.F32, B, m.T, m.D, m.Dm, m.depth, m.num_heads, m.Kp, m.No,
                           m.defer_wgrad, ckpt)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ckpt", [False, True])
def test_workspace_bytes_equal_the_plan(ckpt, dtype, depth):
    m = _run(depth, dtype, ckpt)[0]
    ws = m._ws_cur
    ts = _ws_tensors(ws)
    total = sum(t.numel() * t.element_size() for t in ts)
    plan = _plan_of(m, 4, ckpt)
    assert total == plan.total == ws.nbytes() and len(ts) == len(ws._bufs)
    assert ws.plan.total == plan.total and ws.ckpt == ckpt


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_peak_memory_drops_by_the_plans_difference(dtype):
    """depth 8: torch.cuda.max_memory_allocated over one step (model built and moved first) drops by the difference of the two
    plans, less 512 bytes per workspace tensor for the allocator's rounding."""
    _step(_make(1, dtype, False)), _step(_make(1, dtype, True))            # library-wide scratch pools exist before measuring
    peak, count = {}, {}
    for ckpt in (False, True):
        m = _make(8, dtype, ckpt)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _step(m)
        torch.cuda.synchronize()
        peak[ckpt] = torch.cuda.max_memory_allocated() - before
        count[ckpt] = len(_ws_tensors(m._ws_cur))
        assert m._ws_cur.ckpt == ckpt
        plan = _plan_of(m, 4, ckpt)
        assert plan.total == m._ws_cur.nbytes()
        peak[ckpt, "plan"] = plan.total
        del m
    want = peak[False, "plan"] - peak[True, "plan"]
    print(f"[ckpt memory, {dtype}, depth 8] peak off {peak[False]} on {peak[True]} B; plans {peak[False, 'plan']} / {peak[True, 'plan']} B; "
          f"tensors {count[False]} / {count[True]}")
    assert want > 0
    assert peak[False] - peak[True] >= want - 512 * count[True]


def _run_trainer(model, args, batches, steps, fused):
    ema_model = copy.deepcopy(model)
    if fused:
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule(args.path_type, 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, batches, Pbar())
    losses = [tr.train_step(s) for s in range(1, steps + 1)]
    psum = float(sum(p.double().abs().sum() for p in model.parameters()))
    esum = float(sum(v.double().abs().sum() for v in ema_model.state_dict().values()))
    return losses, psum, esum


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_trajectory_checkpointed_tiny_dit_fp32_vs_reference(fused):
    """test_gpu_dit.py::test_trainer_trajectory_tiny_dit_fp32_vs_reference with args.activation_checkpointing=True: the
    reference Trainer's 6 steps (fixture), 1e-4 relative on every loss."""
    exp = load_json("trainer.json")["dit_tiny_latent"]
    args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, lr=1e-3, cpu_rng=True, activation_checkpointing=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2,
                        class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype="fp32").to(DEV)
    assert not model.activation_checkpointing
    losses, psum, esum = _run_trainer(model, args, synth_loader(8, 8, 8, 3, 10, latent=True), 6, fused)
    assert model.activation_checkpointing and model._ws_cur.ckpt
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)
    assert psum == pytest.approx(exp["param_abs_sum"], rel=1e-5)
    assert esum == pytest.approx(exp["ema_abs_sum"], rel=1e-6)


def test_hip_graph_checkpointed_step_matches_eager_checkpointed_step():
    """test_gpu_dit.py::test_hip_graph_step_matches_eager_step with args.activation_checkpointing=True: the captured step (with
    every block's recomputation and per-block weight-gradient launch in it) replays the eager trajectory bit for bit."""
    class FixedDraws(vaw_amd.GaussianDiffusion):
        def training_losses(self, model, x_start, features=None, t=None, model_kwargs=None, noise=None):
            return super().training_losses(model, x_start, features, t=self._t, model_kwargs=model_kwargs, noise=self._noise)

    def run(graph):
        args = base_args(in_chans=4, class_cond=True, dataset="Pixels4", image_size=8, lr=1e-3, warmup_steps=3, cosine_decay=True,
                         total_steps=20, final_lr=1e-5, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph, amp=True,
                         activation_checkpointing=True)
        args.in_chans = 3            # no latent sampling: Trainer draws nothing itself
        random.seed(42); np.random.seed(42); torch.manual_seed(42)
        model = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=3, num_heads=2,
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
        assert model.activation_checkpointing and model._ws_cur.ckpt and model._ws_cur.defer
        assert (tr._graph is not None) == bool(graph)
        return losses, model._flat.clone(), ema_model._flat.clone(), sched.get_last_lr()[0], opt.step_count

    le, pe, ee, lre, ne = run(False)
    lg, pg, eg, lrg, ng = run(True)
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(ee, eg)
    assert lre == lrg and ne == ng == 8
    assert le[-1] < le[0]


@pytest.mark.parametrize("first", [False, True])
def test_toggling_the_flag_between_forward_and_backward_raises(first):
    m = _make(3, "fp32", first)
    i = _inputs()
    out, _ = m(i["x"].clone().requires_grad_(True), i["t"], i["y"])
    m.set_activation_checkpointing(not first)
    with pytest.raises(vaw_amd.VawError, match="activation_checkpointing"):
        (out * i["gout"]).sum().backward()
    # a fresh forward in the new mode trains as usual
    out, _ = m(i["x"], i["t"], i["y"])
    (out * i["gout"]).sum().backward()
    assert m._ws_cur.ckpt == (not first) and torch.isfinite(m.flat_grads()).all()

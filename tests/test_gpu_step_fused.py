"""The fused passes of the training step (VAW_STEP_FUSED) against the sequences of launches they replace: bit for bit
wherever the arithmetic and its order are kept, and against float64 / the f32 oracle trajectory where a reduction order moved (the
batch means of the loss)."""
import copy
import random

import numpy as np
import pytest
import torch

from conftest import Pbar, base_args, perturb_, synth_loader

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, ptr

DEV = "cuda"
ULP = float(np.finfo(np.float32).eps)


def _diffusion(args=None, **kw):
    kw = dict(dict(model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                   loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True), **kw)
    return vaw_amd.GaussianDiffusion(args=args or base_args(in_chans=4, class_cond=True),
                                     betas=vaw_amd.get_named_beta_schedule("cosine", 1000), **kw)


def _t_with_ends(B, g):
    """B timesteps that contain 0 and 999 (B = 1: the caller runs both)."""
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0] = 0
    t[-1] = 999 if B > 1 else t[-1]
    return t


# (B, C, hw): 4 x 32 x 32 and 4 x 6 x 6 (a grid tail), and 3 x 5 x 5 = 75 elements per sample: the scalar loops of the kernels
SHAPES = [(B, 4, hw) for B in (1, 3, 8) for hw in (32, 6)] + [(3, 3, 5)]


@pytest.mark.parametrize("B,C,hw", SHAPES)
def test_latent_qsample_is_bitwise_the_tensor_chain(B, C, hw):
    g = torch.Generator().manual_seed(100 * B + hw)
    tb = _diffusion()._tables(torch.device(DEV))
    latent = torch.cat([torch.randn(B, C, hw, hw, generator=g) * 4, torch.rand(B, C, hw, hw, generator=g) * 1.45 + 0.05], 1).to(DEV)
    eps, noise = torch.randn(B, C, hw, hw, generator=g).to(DEV), torch.randn(B, C, hw, hw, generator=g).to(DEV)
    for t in ([_t_with_ends(B, g)] if B > 1 else [torch.tensor([0]), torch.tensor([999])]):
        t = t.to(DEV)
        mean, std = torch.chunk(latent, 2, dim=1)
        x0_ref = (mean + std * eps) * 0.18215                       # sample_from_latent on the same eps
        xt_ref = ops.qsample(x0_ref.contiguous(), noise, t, tb["a"], tb["s"])
        for t_scale in (1.0, 0.25):
            x0, x_t, tf = ops.latent_qsample(latent, eps, noise, t, tb["a"], tb["s"], 0.18215, t_scale)
            assert torch.equal(x0, x0_ref) and torch.equal(x_t, xt_ref)
            assert torch.equal(tf, t.float() * t_scale)
        x0, x_t = ops.latent_qsample(latent, eps, noise, t, tb["a"], tb["s"], 0.18215)
        assert torch.equal(x0, x0_ref) and torch.equal(x_t, xt_ref)
    bad = torch.full((B,), 1000, dtype=torch.int64, device=DEV)     # out of range: the row is poisoned, as vaw_qsample_fwd does
    assert torch.isnan(ops.latent_qsample(latent, eps, noise, bad, tb["a"], tb["s"], 1.0)[1]).all()


@pytest.mark.parametrize("B,C,hw", SHAPES)
def test_fused_loss_terms_gradient_and_batch_mean(B, C, hw):
    g = torch.Generator().manual_seed(7 * B + hw)
    tb = _diffusion(model_mean_type=vaw_amd.ModelMeanType.VELOCITY)._tables(torch.device(DEV))     # ca, cb, w all non-trivial
    x0, noise, out = (torch.randn(B, C, hw, hw, generator=g).to(DEV) for _ in range(3))
    for t in ([_t_with_ends(B, g)] if B > 1 else [torch.tensor([0]), torch.tensor([999])]):
        t = t.to(DEV)
        ca, cb, w = tb["ca"][t], tb["cb"][t], tb["w"][t]
        for accum in (1, 2):
            o_ref = out.clone().requires_grad_(True)
            mse_ref = ops.weighted_mse(o_ref, x0, noise, ca, cb, w)
            mean_ref = mse_ref.mean() / accum
            mean_ref.backward()
            o = out.clone().requires_grad_(True)
            mse, mean = ops.weighted_mse_mean(o, x0, noise, t, tb["ca"], tb["cb"], tb["w"], accum)
            torch.autograd.backward(mean, ops.one_like(mean))
            assert torch.equal(mse, mse_ref.detach()) and not mse.requires_grad
            if accum == 1:
                assert torch.equal(o.grad, o_ref.grad)
            else:       # the kernel rounds g / (B accum) * w * 2 / n once more than the chain does at most: 1 ulp per element
                assert float(((o.grad - o_ref.grad).abs() / o_ref.grad.abs().clamp_min(1e-30)).max()) <= ULP
            # batch mean against float64; allowed = 4 x the error of the tensor-operation path on the same inputs, floor 2 ulp
            exact = float(mse_ref.detach().double().mean() / accum)
            e_new, e_old = abs(float(mean.detach()) - exact), abs(float(mean_ref.detach()) - exact)
            print(f"batch mean B={B} C={C} hw={hw} accum={accum}: fused {e_new / abs(exact) / ULP:.2f} ulp, tensor ops {e_old / abs(exact) / ULP:.2f} ulp")
            assert e_new <= max(4 * e_old, 2 * ULP * abs(exact))
        # per-row coefficients (t = None: the flow-matching objective) take the same kernel
        o = out.clone().requires_grad_(True)
        mse, mean = ops.weighted_mse_mean(o, x0, noise, None, ca.contiguous(), cb.contiguous(), w.contiguous(), 1)
        torch.autograd.backward(mean, ops.one_like(mean))
        assert torch.equal(mse, mse_ref.detach()) and torch.equal(o.grad, _grad_at_accum1(out, x0, noise, ca, cb, w))


def _grad_at_accum1(out, x0, noise, ca, cb, w):
    o = out.clone().requires_grad_(True)
    ops.weighted_mse(o, x0, noise, ca, cb, w).mean().backward()
    return o.grad


@pytest.mark.parametrize("M,N", [(3, 1536), (8, 56832), (256, 1024)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_cast_colsum_is_bitwise_cast_then_colsum(M, N, beta):
    g = torch.Generator().manual_seed(M + N)
    src = (torch.randn(M, N, generator=g) * 3).to(DEV)
    src[0, :8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 65504.0, 1.00390625, -1.00390625, 3e38])       # zeros, ties, near overflow
    prev = torch.randn(N, generator=g).to(DEV)
    dst_ref, dst = (torch.zeros((M + 63) // 64 * 64, N, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    ops.cast_bf16(src, dst_ref)
    cs_ref = prev.clone()
    ops.colsum(BF16, ptr(dst_ref), M, N, N, ptr(cs_ref), beta)
    cs = prev.clone()
    assert ops.cast_colsum_plan(M, N, N, N, ptr(src), ptr(dst), ptr(cs)) is not None
    ops.cast_colsum(ptr(src), N, ptr(dst), N, M, N, ptr(cs), beta)
    assert torch.equal(dst.view(torch.int16), dst_ref.view(torch.int16)) and torch.equal(cs.view(torch.int32), cs_ref.view(torch.int32))
    # a column window of a wider matrix (the early adaLN bucket): only the window is written
    if N >= 1536:
        c0, n = 512, 768
        dst2, cs2 = torch.zeros_like(dst), prev.clone()
        ops.cast_colsum(ptr(src) + 4 * c0, N, ptr(dst2) + 2 * c0, N, M, n, ptr(cs2) + 4 * c0, beta)
        assert torch.equal(dst2[:M, c0:c0 + n].view(torch.int16), dst_ref[:M, c0:c0 + n].view(torch.int16))
        assert torch.equal(cs2[c0:c0 + n], cs_ref[c0:c0 + n]) and torch.equal(cs2[:c0], prev[:c0]) and torch.equal(cs2[c0 + n:], prev[c0 + n:])
        assert float(dst2[:, :c0].float().abs().max()) == 0.0 and float(dst2[:, c0 + n:].float().abs().max()) == 0.0


def test_cast_colsum_refuses_what_it_does_not_cover():
    src, dst, cs = torch.zeros(600, 64, device=DEV), torch.zeros(640, 64, device=DEV, dtype=torch.bfloat16), torch.ones(64, device=DEV)
    for M, N, ld, so, do in ((600, 64, 64, 0, 0), (8, 62, 64, 0, 0), (8, 64, 66, 0, 0), (8, 32, 64, 4, 0), (8, 32, 64, 0, 8)):
        assert ops.cast_colsum_plan(M, N, ld, ld, ptr(src) + so, ptr(dst) + do, ptr(cs)) is None
        with pytest.raises(vaw_amd.VawError):
            ops.cast_colsum(ptr(src) + so, ld, ptr(dst) + do, ld, M, N, ptr(cs), 0.0)
    torch.cuda.synchronize()
    assert float(dst.float().abs().max()) == 0.0 and float((cs - 1).abs().max()) == 0.0          # nothing was launched


@pytest.mark.parametrize("D", [384, 768])
def test_extra_act_outputs_of_silu_bwd_and_ln_bwd(D):
    g = torch.Generator().manual_seed(D)
    B, T = 2, 64
    M = B * T
    # silu_bwd: [B*T, D]
    x, dy = torch.randn(M, D, generator=g).to(DEV), torch.randn(M, D, generator=g).to(DEV)
    dx_ref, dx, dxa = torch.empty_like(x), torch.empty_like(x), torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
    L.check(L.lib().vaw_silu_bwd(ptr(x), ptr(dy), ptr(dx_ref), M * D, L.stream_ptr()), "silu_bwd")
    ops.silu_bwd(x, dy, dx, dxa)
    ref_a = torch.empty_like(dxa)
    ops.cast_bf16(dx_ref, ref_a)
    assert torch.equal(dx, dx_ref) and torch.equal(dxa.view(torch.int16), ref_a.view(torch.int16))
    dx2 = torch.empty_like(x)
    ops.silu_bwd(x, dy, dx2, None)
    assert torch.equal(dx2, dx_ref)
    # LayerNorm + modulate backward, both act dtypes
    for dt, tdt in ((BF16, torch.bfloat16), (F32, torch.float32)):
        ld = 2 * D
        dout = torch.randn(M, D, generator=g).to(DEV).to(tdt)
        xin, dres_in = torch.randn(M, D, generator=g).to(DEV), torch.randn(M, D, generator=g).to(DEV)
        mean, rstd = xin.mean(1).contiguous(), (xin.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
        mod = torch.randn(B, ld, generator=g).to(DEV)

        def run(dx_act):
            dx, dmod = torch.empty(M, D, device=DEV), torch.zeros(B, ld, device=DEV)
            ops.ln_modulate_bwd(dt, ptr(dout), ptr(xin), ptr(mean), ptr(rstd), ptr(mod) + 4 * D, ld, ptr(dres_in), ptr(dx), ptr(dmod),
                                ptr(dmod) + 4 * D, ld, B, T, D, dx_act=ptr(dx_act))
            return dx, dmod

        dx_ref, dmod_ref = run(None)
        act = torch.empty(M, D, device=DEV, dtype=tdt)
        dx, dmod = run(act)
        assert torch.equal(dx, dx_ref) and torch.equal(dmod, dmod_ref)          # the f32 outputs do not move
        if dt == BF16:
            ref_a = torch.empty_like(act)
            ops.cast_bf16(dx_ref, ref_a)
            assert torch.equal(act.view(torch.int16), ref_a.view(torch.int16))
        else:
            assert torch.equal(act, dx_ref)


@pytest.mark.parametrize("B,D,rows", [(8, 64, 11), (256, 768, 1001), (1100, 260, 5)])
def test_embedding_bwd_adds_matching_rows_in_batch_order(B, D, rows):
    g = torch.Generator().manual_seed(B)
    dc = torch.randn(B, D, generator=g)
    idx = torch.randint(0, rows, (B,), generator=g)
    idx[: min(B, 4)] = rows - 1                                   # a row hit several times, the last table row
    prev = torch.randn(rows, D, generator=g)
    for beta in (0.0, 1.0):
        ref = prev.clone() * beta if beta else torch.zeros_like(prev)
        acc = torch.zeros(rows, D)
        for b in range(B):                                        # b ascending, f32: the kernel's order
            acc[idx[b]] += dc[b]
        ref = ref + acc
        tab, dc_d, idx_d = prev.clone().to(DEV), dc.to(DEV), idx.to(DEV)
        L.check(L.lib().vaw_embedding_bwd(ptr(dc_d), ptr(idx_d), ptr(tab), B, D, rows, beta, L.stream_ptr()), "embedding_bwd")
        assert torch.equal(tab.cpu(), ref)


# ---- whole steps -------------------------------------------------------------------------------------------------------------
def _model_kw(name):
    if name in ("p2", "p4"):
        return dict(image_size=8, patch_size=int(name[1]), in_channels=4, hidden_size=64, depth=4, num_heads=2, class_dropout_prob=0.0,
                    num_classes=10, learn_sigma=False), 8
    return dict(image_size=32, patch_size=4, in_channels=4, hidden_size=384, depth=12, num_heads=6, class_dropout_prob=0.0,
                num_classes=10, learn_sigma=False), 32


def _args(hw, **kw):
    return base_args(**dict(dict(in_chans=4, class_cond=True, dataset="Latent", image_size=hw, lr=1e-3, amp=True, cpu_rng=True), **kw))


def _hip_steps(name, monkeypatch, fused, steps=3, hook=False, dtype="bf16", rescale=True, **akw):
    monkeypatch.setattr(L, "STEP_FUSED", bool(fused))
    kw, hw = _model_kw(name)
    args = _args(hw, **akw)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(compute_dtype=dtype, **kw)
    perturb_(model, 5)
    model = model.to(DEV)
    seen = []
    if hook:
        model.grad_ready_hook = seen.append
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    accum = max(1, args.grad_accumulation)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, _diffusion(args, rescale_timesteps=rescale), synth_loader(8, 8, hw, 3 * accum, 10, latent=True), Pbar())
    assert tr._fused_latent == bool(fused)
    torch.manual_seed(7)
    losses = [float(tr.train_step(s)) for s in range(1, steps + 1)]
    if hook:
        assert seen and seen[-1] == 0
    params = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters() if p.requires_grad])      # registration order
    return losses, model._flat.detach().clone(), ema_model._flat.detach().clone(), params


_ORACLE = {}


def _oracle_steps(name, steps=3, **akw):
    """The same steps of the f32 CPU oracle (same weights, same CPU generator stream); computed once per configuration."""
    key = (name, steps, tuple(sorted(akw.items())))
    if key not in _ORACLE:
        from oracle import diffusion as od, dit as odit, trainer as otr
        kw, hw = _model_kw(name)
        args = _args(hw, amp=False, **akw)
        random.seed(42); np.random.seed(42); torch.manual_seed(42)
        model = odit.DiT(**kw)
        perturb_(model, 5)
        ema_model = copy.deepcopy(model)
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = od.GaussianDiffusion(args=args, betas=od.get_named_beta_schedule("cosine", 1000), model_mean_type=od.ModelMeanType.EPSILON,
                                    model_var_type=od.ModelVarType.FIXED_LARGE, loss_type=od.LossType.MSE, rescale_timesteps=True)
        accum = max(1, args.grad_accumulation)
        tr = otr.Trainer(args, torch.device("cpu"), model, ema_model, opt, sched, diff, synth_loader(8, 8, hw, 3 * accum, 10, latent=True), Pbar())
        torch.manual_seed(7)
        losses = [float(tr.train_step(s)) for s in range(1, steps + 1)]
        _ORACLE[key] = (losses, torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad]))
    return _ORACLE[key]


def _distances(run, oracle):
    """(largest relative loss distance, relative L2 distance of the trained weights) of a HIP run to the oracle trajectory."""
    lo, wo = oracle
    dl = max(abs(a - b) / abs(b) for a, b in zip(run[0], lo))
    w = run[3].double()
    assert w.shape == wo.shape
    return dl, float((w - wo.double()).norm() / wo.double().norm())


@pytest.mark.parametrize("name", ["p2", "p4", "dit_s4"])
def test_three_steps_fused_against_unfused(name, monkeypatch):
    """accum = 1, bf16: every fused pass keeps its values but the batch mean of the loss (one fixed-order launch instead of a
    tensor reduction), and that mean does not feed the gradient.  So the weights are bitwise those of VAW_STEP_FUSED=0, and the
    reported losses stay as close to the f32 oracle trajectory (within the 10 % headroom a changed reduction order is given)."""
    fused, plain = _hip_steps(name, monkeypatch, True), _hip_steps(name, monkeypatch, False)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    oracle = _oracle_steps(name)
    (dlf, dwf), (dlp, dwp) = _distances(fused, oracle), _distances(plain, oracle)
    print(f"{name}: loss distance to the oracle fused {dlf:.3e} unfused {dlp:.3e}; weights fused {dwf:.3e} unfused {dwp:.3e}")
    assert dlf <= 1.1 * dlp and dwf == dwp
    for a, b in zip(fused[0], plain[0]):
        assert abs(a - b) <= 4 * ULP * abs(b)


@pytest.mark.parametrize("name", ["p2", "dit_s4"])
def test_three_steps_fused_with_hook_accumulation_and_clip(name, monkeypatch):
    # a gradient-ready listener (the early adaLN bucket: two column windows of the fused cast + column sums): bitwise
    fused, plain = _hip_steps(name, monkeypatch, True, hook=True), _hip_steps(name, monkeypatch, False, hook=True)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    # gradient clipping: the norm is taken of bitwise the same gradients
    fused, plain = _hip_steps(name, monkeypatch, True, grad_clip=0.5), _hip_steps(name, monkeypatch, False, grad_clip=0.5)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    # accumulation over two micro-batches: the loss gradient is within 1 ulp of the chain's, so the standard is the oracle distance
    fused, plain = _hip_steps(name, monkeypatch, True, grad_accumulation=2), _hip_steps(name, monkeypatch, False, grad_accumulation=2)
    oracle = _oracle_steps(name, grad_accumulation=2)
    (dlf, dwf), (dlp, dwp) = _distances(fused, oracle), _distances(plain, oracle)
    print(f"{name} accum 2: loss distance fused {dlf:.3e} unfused {dlp:.3e}; weights fused {dwf:.3e} unfused {dwp:.3e}")
    assert dlf <= 1.1 * dlp and dwf <= 1.1 * dwp


def test_three_steps_under_hip_graph_equal_eager_fused(monkeypatch):
    """The fused step captured into one graph (device RNG: the philox offsets of eager and replayed draws advance alike) gives the
    eager fused steps bit for bit: no host synchronisation, allocation or upload hides in the new launches."""
    def run(graph):
        torch.cuda.manual_seed(1234)
        return _hip_steps("p2", monkeypatch, True, steps=5, cpu_rng=False, hip_graph=graph, defer_loss_sync=True)

    eager, graph = run(False), run(True)
    assert eager[0] == graph[0], (eager[0], graph[0])
    assert torch.equal(eager[1], graph[1]) and torch.equal(eager[2], graph[2])


def test_f32_parity_mode_is_untouched_by_the_switch(monkeypatch):
    """fp32 compute: the conversions do not exist; the latent sample and the loss take the fused launches, bitwise."""
    fused, plain = _hip_steps("p2", monkeypatch, True, dtype="fp32", amp=False), _hip_steps("p2", monkeypatch, False, dtype="fp32", amp=False)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])


def test_without_rescale_timesteps_the_model_still_gets_int64_t(monkeypatch):
    """rescale_timesteps=False: _scale_timesteps hands the model the int64 t itself, and so does the fused step (the kernel writes no
    scaled copy); the steps stay bitwise those of the unfused sequence."""
    seen = []
    orig = vaw_amd.DiT.forward
    monkeypatch.setattr(vaw_amd.DiT, "forward", lambda self, x, t, y, **kw: (seen.append(t.dtype), orig(self, x, t, y, **kw))[1])
    fused, plain = _hip_steps("p2", monkeypatch, True, rescale=False), _hip_steps("p2", monkeypatch, False, rescale=False)
    assert seen and all(d == torch.int64 for d in seen)
    assert fused[0] == plain[0] or all(abs(a - b) <= 4 * ULP * abs(b) for a, b in zip(fused[0], plain[0]))
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])


def test_fused_step_launches_no_tensor_kernel_for_the_anchor_or_the_loss(monkeypatch):
    """The DiT node's anchor gets no gradient in the fused step (no fill, no accumulate), and the loss node's per-sample output no
    materialised zeros."""
    monkeypatch.setattr(L, "STEP_FUSED", True)
    kw, hw = _model_kw("p2")
    m = vaw_amd.DiT(compute_dtype="bf16", **kw).to(DEV)
    perturb_(m, 5)
    g = torch.Generator().manual_seed(3)
    x, t, y = torch.randn(4, 4, hw, hw, generator=g).to(DEV), torch.rand(4, generator=g).to(DEV) * 999, torch.randint(0, 10, (4,), generator=g).to(DEV)
    for _ in range(2):
        out, _ = m(x, t, y)
        out.sum().backward()
    assert m._anchor.grad is None and float(m.flat_grads().abs().max()) > 0

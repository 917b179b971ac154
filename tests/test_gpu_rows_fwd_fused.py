"""vaw_gate_resid_ln_modulate_fwd (csrc/layernorm.hip: the gated residual add of a DiT branch and the LayerNorm + modulate behind
it in one row pass) and the bf16 block forward that uses it (VAW_ROWS_FWD_FUSED).

  * the kernel against float64 over every NV bucket, a masked tail lane, row counts that are no multiple of the waves of a grid pass,
    modulation strides and offsets as dit.py passes them, and the residual-only mode.  Tolerances are those of
    tests/test_gpu_rows.py for vaw_ln_modulate_fwd at the same D (imported from there); x_out, an f32 output, takes its f32 rule;
  * bitwise against the pair it replaces -- vaw_gemm with the gated-residual epilogue + vaw_ln_modulate_fwd -- with y from the same
    GEMM with a plain store.  The GEMM kernels do not round y * gate + x alike: the persistent kernel's epilogue is one fma
    (v_pk_fma_f32 in gemm_p8_kernel<.., P8_GATE, ..>), the 64-row and 128-row kernels round the product first (epi_row8:
    v_pk_mul_f32, then v_pk_add_f32 in another basic block).  vaw_gemm hands both small shapes named for this test (M = 512,
    D = K = 768 and M = 128, D = K = 256) to the small-M kernel, so a third, M = 8256, covers the persistent one.  The row pass
    rounds as the kernel of the gated launch does (vaw_gate_resid_fwd_contracts), and all three are bitwise;
  * refusals: nothing is launched;
  * whole training steps, recomputation, the EMA model's eval forward and a captured step with the switch on and off: bitwise."""
import copy
import random

import numpy as np
import pytest
import torch

from conftest import Pbar, base_args, perturb_, synth_loader
from test_gpu_rows import EPS, _close_bf16, _close_f32, _rms      # the tolerances of vaw_ln_modulate_fwd against float64

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, lib, ptr, stream_ptr

DEV = "cuda"
WIDTHS = [4, 252, 256, 260, 768, 1152, 1280, 2048]
# (33, 257): 8481 rows, more than four times the 2048 workgroups of the widest resident round (NV = 1: 8 per CU), so at every width
# waves walk more than one row, with a short last pass; the other row counts stay below one round (one row per wave)
ROWS = [(1, 1), (3, 7), (2, 64), (5, 33), (33, 257)]


def _nv(D):
    nv = -(-D // 256)
    return nv if nv <= 6 else 8


def _call(y, mod, g_o, sh_o, sc_o, mod_ld, x, xo, out, mean, rstd, B, T, D, dt=BF16):
    return lib().vaw_gate_resid_ln_modulate_fwd(dt, ptr(y), ptr(mod) + 4 * g_o, mod_ld, ptr(x), ptr(xo), ptr(mod) + 4 * sh_o, ptr(mod) + 4 * sc_o,
                                                mod_ld, ptr(out) or None, ptr(mean) or None, ptr(rstd) or None, B, T, D, EPS, stream_ptr())


@pytest.mark.parametrize("B,T", ROWS)
@pytest.mark.parametrize("D", WIDTHS)
def test_kernel_vs_float64(D, B, T):
    M = B * T
    ci = WIDTHS.index(D) * len(ROWS) + ROWS.index((B, T))
    depth = 3
    mod_ld, base = ((6 * D, 0), ((6 * depth + 2) * D, 6 * D))[ci % 2]      # dit.py: block l's six chunks at 6*l*D of (6*depth+2)*D
    g_o, sh_o, sc_o = ((base + 2 * D, base + 3 * D, base + 4 * D), (base + 5 * D, base, base + D))[(ci // 2) % 2]     # proj site | fc2 site
    p = ops.row_plan(L.ROW_GATE_LN_FWD, BF16, B, T, D, ldx=mod_ld)
    assert (p.variant, p.nv, p.block, p.lds_bytes) == (L.RV_GATE_LN_FWD, _nv(D), 256, 0) and p.grid_x == -(-M // 4)
    assert (M > 4 * 2048) == ((B, T) == ROWS[-1])
    g = torch.Generator().manual_seed(D * 7 + T)
    y_h = torch.randn(M, D, generator=g).bfloat16()
    x_h, mod_h = torch.randn(M, D, generator=g) * 2 + 0.5, torch.randn(B, mod_ld, generator=g) * 0.5
    y, x, mod = y_h.to(DEV), x_h.to(DEV), mod_h.to(DEV)
    tag = f"D={D} B={B} T={T} mod_ld={mod_ld} gate@{g_o} shift@{sh_o} scale@{sc_o}"

    def run(ln):
        xo = torch.full((M, D), 7.0, device=DEV)
        out = torch.full((M, D), 7.0, device=DEV, dtype=torch.bfloat16)
        mean, rstd = torch.full((M,), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV)
        ops.check(_call(y, mod, g_o, sh_o, sc_o, mod_ld, x, xo, out if ln else None, mean if ln else None, rstd if ln else None, B, T, D),
                  "vaw_gate_resid_ln_modulate_fwd")
        torch.cuda.synchronize()
        return xo, out, mean, rstd

    full, again, resid = run(True), run(True), run(False)
    for u, v in zip(full, again):
        assert torch.equal(u, v), "two runs of the same call differ: " + tag
    xo, out, mean, rstd = full
    gate, shift, scale = (mod_h[:, o:o + D].double() for o in (g_o, sh_o, sc_o))
    xr = (y_h.double().view(B, T, D) * gate[:, None] + x_h.double().view(B, T, D)).reshape(M, D)
    _close_f32(xo, xr, 1e-5 * _rms(xr), "x_out " + tag)
    ref_out = (torch.nn.functional.layer_norm(xr, (D,), eps=EPS).view(B, T, D) * (1 + scale[:, None]) + shift[:, None]).reshape(M, D)
    _close_bf16(out, ref_out, 1e-5 * _rms(ref_out), "out " + tag)
    _close_f32(mean, xr.mean(1), 1e-5 * _rms(xr), "mean " + tag)
    ref_rstd = 1.0 / torch.sqrt(xr.var(1, unbiased=False) + EPS)
    _close_f32(rstd, ref_rstd, 1e-5 * _rms(ref_rstd), "rstd " + tag)
    # out == NULL: the same residual, and the LayerNorm outputs are not touched
    assert torch.equal(resid[0], xo), tag
    assert float((resid[1].float() - 7).abs().max()) == 0.0 and float((resid[2] - 7).abs().max()) == 0.0 and float((resid[3] - 7).abs().max()) == 0.0
    # the LayerNorm half is vaw_ln_modulate_fwd on the same x_out, bit for bit
    out2, mean2, rstd2 = torch.empty_like(out), torch.empty_like(mean), torch.empty_like(rstd)
    ops.ln_modulate_fwd(BF16, ptr(xo), ptr(mod) + 4 * sh_o, ptr(mod) + 4 * sc_o, mod_ld, ptr(out2), ptr(mean2), ptr(rstd2), B, T, D, EPS)
    assert torch.equal(out2, out) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd), tag


@pytest.mark.parametrize("M,D,K", [(512, 768, 768), (128, 256, 256), (8256, 768, 768)])
def test_bitwise_the_gated_gemm_epilogue_then_ln(M, D, K):
    """y, x_out, out, mean and rstd of the two sequences are bitwise equal on the small-M kernel's rounding (two shapes) and on the
    persistent kernel's (M = 8256); the LayerNorm half alone is vaw_ln_modulate_fwd on the same x_out; two runs are equal."""
    T = 64 if M % 64 == 0 else M
    B = M // T
    ld = 6 * D
    g = torch.Generator().manual_seed(M + D)
    a = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(D, K, generator=g) * K ** -0.5).bfloat16().to(DEV)
    bias, x, mod = torch.randn(D, generator=g).to(DEV), (torch.randn(M, D, generator=g) * 2).to(DEV), (torch.randn(B, ld, generator=g) * 0.5).to(DEV)
    gate, shift, scale = ptr(mod) + 4 * 2 * D, ptr(mod) + 4 * 3 * D, ptr(mod) + 4 * 4 * D

    def pair():
        y, xo = torch.empty(M, D, device=DEV, dtype=torch.bfloat16), torch.empty(M, D, device=DEV)
        out, mean, rstd = torch.empty_like(y), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        ops.gemm(BF16, 1, 1, M, D, K, ptr(a), K, ptr(w), K, ptr(xo), D, bias=ptr(bias), aux_out=ptr(y), gate=gate, gate_ld=ld, resid=ptr(x),
                 rows_per_batch=T, out_f32=True)
        ops.ln_modulate_fwd(BF16, ptr(xo), shift, scale, ld, ptr(out), ptr(mean), ptr(rstd), B, T, D, EPS)
        torch.cuda.synchronize()
        return y, xo, out, mean, rstd

    def fused():
        y, xo = torch.empty(M, D, device=DEV, dtype=torch.bfloat16), torch.empty(M, D, device=DEV)
        out, mean, rstd = torch.empty_like(y), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        ops.gemm(BF16, 1, 1, M, D, K, ptr(a), K, ptr(w), K, ptr(y), D, bias=ptr(bias))
        ops.gate_resid_ln_modulate_fwd(BF16, ptr(y), gate, ld, ptr(x), ptr(xo), shift, scale, ld, ptr(out), ptr(mean), ptr(rstd), B, T, D, EPS)
        torch.cuda.synchronize()
        return y, xo, out, mean, rstd

    p = ops.gemm_plan(BF16, 1, 1, M, D, K, ptr(a), K, ptr(w), K, ptr(x), D, bias=ptr(bias), aux_out=ptr(a), gate=gate, gate_ld=ld, resid=ptr(x),
                      rows_per_batch=T, out_f32=True)
    ref, got, again = pair(), fused(), fused()
    for u, v in zip(got, again):
        assert torch.equal(u, v), "two runs of the fused sequence differ"
    diff = ref[1] != got[1]
    ulps = (ref[1].view(torch.int32) - got[1].view(torch.int32)).abs()
    print(f"M={M} D={D} K={K}: gated launch on {L.GV_NAMES[p.variant]}; x_out differs in {int(diff.sum())} / {diff.numel()} elements, "
          f"at most {int(ulps.max())} ulp; out differs in {int((ref[2] != got[2]).sum())}, mean in {int((ref[3] != got[3]).sum())}, "
          f"rstd in {int((ref[4] != got[4]).sum())}")
    assert (p.variant == L.GV_PERSISTENT) == (M > 8192) == bool(lib().vaw_gate_resid_fwd_contracts(B, T, D))
    assert torch.equal(ref[0], got[0]), "y"
    # the LayerNorm half alone: vaw_ln_modulate_fwd on the fused sequence's x_out
    out2, mean2, rstd2 = torch.empty_like(got[2]), torch.empty_like(got[3]), torch.empty_like(got[4])
    ops.ln_modulate_fwd(BF16, ptr(got[1]), shift, scale, ld, ptr(out2), ptr(mean2), ptr(rstd2), B, T, D, EPS)
    assert torch.equal(out2, got[2]) and torch.equal(mean2, got[3]) and torch.equal(rstd2, got[4])
    for name, u, v in zip(("x_out", "out", "mean", "rstd"), ref[1:], got[1:]):
        assert torch.equal(u, v), name


def test_refusals_launch_nothing():
    B, T, D = 2, 8, 64
    M = B * T
    y = torch.zeros(M + 1, D, device=DEV, dtype=torch.bfloat16)
    x, mod = torch.zeros(M + 1, D, device=DEV), torch.zeros(B, 6 * D, device=DEV)
    xo, out = torch.full((M + 1, D), 7.0, device=DEV), torch.full((M + 1, D), 7.0, device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.full((M,), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV)
    f = lib().vaw_gate_resid_ln_modulate_fwd
    ok = dict(dt=BF16, y=ptr(y), gate=ptr(mod) + 8 * D, gate_ld=6 * D, x=ptr(x), xo=ptr(xo), sh=ptr(mod) + 12 * D, sc=ptr(mod) + 16 * D, mod_ld=6 * D,
              out=ptr(out), D=D)
    bad = [dict(D=62), dict(y=ptr(y) + 8), dict(x=ptr(x) + 4), dict(xo=ptr(xo) + 8), dict(out=ptr(out) + 8), dict(gate=ptr(mod) + 8),
           dict(gate_ld=6 * D + 2), dict(mod_ld=6 * D + 1), dict(dt=F32), dict(dt=L.FP8), dict(xo=ptr(x))]
    for change in bad:
        a = dict(ok, **change)
        rc = f(a["dt"], a["y"], a["gate"], a["gate_ld"], a["x"], a["xo"], a["sh"], a["sc"], a["mod_ld"], a["out"], ptr(mean), ptr(rstd), B, T, a["D"],
               EPS, stream_ptr())
        assert rc == -1, (change, rc)                   # VAW_ERR_INVALID
        assert lib().vaw_last_error_string()
    rc = f(BF16, ptr(y), ptr(mod), 6 * D, ptr(x), ptr(xo), None, None, 6 * D, ptr(out), ptr(mean), ptr(rstd), B, T, D, EPS, stream_ptr())
    assert rc == -1                                     # out without its modulation rows
    torch.cuda.synchronize()
    for t in (xo, out.float(), mean, rstd):
        assert float((t - 7).abs().max()) == 0.0        # nothing was launched
    with pytest.raises(vaw_amd.VawError):
        ops.row_plan(L.ROW_GATE_LN_FWD, F32, B, T, D)


# ---- whole steps -------------------------------------------------------------------------------------------------------------
def _model_kw(name):
    """-> (DiT arguments, image size, batch).  b4w: DiT-B/4's widths at two blocks and 136 images -- 8704 token rows, the smallest
    round batch at which vaw_gemm gives proj and fc2 to the persistent kernel, so the block forward takes the row pass."""
    if name in ("p2", "p4"):
        return dict(image_size=8, patch_size=int(name[1]), in_channels=4, hidden_size=64, depth=4, num_heads=2, class_dropout_prob=0.0,
                    num_classes=10, learn_sigma=False), 8, 8
    if name == "dit_s4":
        return dict(image_size=32, patch_size=4, in_channels=4, hidden_size=384, depth=12, num_heads=6, class_dropout_prob=0.0,
                    num_classes=10, learn_sigma=False), 32, 8
    return dict(image_size=32, patch_size=4, in_channels=4, hidden_size=768, depth=2, num_heads=12, class_dropout_prob=0.0,
                num_classes=10, learn_sigma=False), 32, 136


def _count_row_passes(monkeypatch):
    calls = []
    orig = ops.gate_resid_ln_modulate_fwd
    monkeypatch.setattr(ops, "gate_resid_ln_modulate_fwd", lambda *a, **k: (calls.append(bool(a[9])), orig(*a, **k))[1])
    return calls


def _steps(name, monkeypatch, fused, steps=3, ckpt=False, **akw):
    """-> (losses, weights, EMA weights, eval output of the EMA model, row passes launched)"""
    monkeypatch.setattr(L, "ROWS_FWD_FUSED", bool(fused))
    calls = _count_row_passes(monkeypatch)
    kw, hw, batch = _model_kw(name)
    args = base_args(**dict(dict(in_chans=4, class_cond=True, dataset="Latent", image_size=hw, lr=1e-3, amp=True, cpu_rng=True), **akw))
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.DiT(compute_dtype="bf16", activation_checkpointing=ckpt, **kw)
    perturb_(model, 5)
    model = model.to(DEV)
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                     model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, synth_loader(batch, 8, hw, 3, 10, latent=True), Pbar())
    torch.manual_seed(7)
    losses = [float(tr.train_step(s)) for s in range(1, steps + 1)]
    g = torch.Generator().manual_seed(11)
    x, t, y = torch.randn(batch, 4, hw, hw, generator=g).to(DEV), (torch.rand(batch, generator=g) * 999).to(DEV), torch.randint(0, 10, (batch,), generator=g).to(DEV)
    ema_model.eval()
    with torch.no_grad():
        ev = ema_model(x, t, y)[0].clone()
    return losses, model._flat.detach().clone(), ema_model._flat.detach().clone(), ev, list(calls)


def _same(on, off):
    assert on[0] == off[0], (on[0], off[0])
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2]) and torch.equal(on[3], off[3])


@pytest.mark.parametrize("ckpt", [False, True], ids=["records", "recompute"])
@pytest.mark.parametrize("name", ["p2", "p4", "dit_s4", "b4w"])
def test_three_steps_and_eval_forward_on_vs_off(name, ckpt, monkeypatch):
    """Losses, weights, EMA and the EMA model's eval forward are bitwise those of VAW_ROWS_FWD_FUSED=0.  At DiT-B/4's widths and
    8704 token rows the row pass runs (twice per block and forward; a recomputed block runs its proj site only); the small
    models keep the GEMM epilogue on their 64-row kernel (DiT._rows_fwd_sites), and launch none."""
    on, off = _steps(name, monkeypatch, True, ckpt=ckpt), _steps(name, monkeypatch, False, ckpt=ckpt)
    _same(on, off)
    assert not off[4]
    if name == "b4w":
        depth, fwd = 2, 3 + 1                               # three training forwards and the eval forward
        assert len(on[4]) == 2 * depth * fwd + (depth * 3 if ckpt else 0) and all(on[4])
    else:
        assert not on[4]


@pytest.mark.parametrize("name", ["p2", "b4w"])
def test_captured_step_equals_eager_step(name, monkeypatch):
    def run(graph):
        torch.cuda.manual_seed(1234)
        return _steps(name, monkeypatch, True, steps=5, cpu_rng=False, hip_graph=graph, defer_loss_sync=True)

    _same(run(True), run(False))


def test_f32_and_fp8_modes_never_take_the_row_pass(monkeypatch):
    monkeypatch.setattr(L, "ROWS_FWD_FUSED", True)
    calls = _count_row_passes(monkeypatch)
    kw, hw, batch = _model_kw("b4w")
    g = torch.Generator().manual_seed(3)
    x, t, y = torch.randn(batch, 4, hw, hw, generator=g).to(DEV), (torch.rand(batch, generator=g) * 999).to(DEV), torch.randint(0, 10, (batch,), generator=g).to(DEV)
    for dtype in ("fp32", "fp8"):
        m = vaw_amd.DiT(compute_dtype=dtype, **dict(kw, depth=1))
        perturb_(m, 5)
        m = m.to(DEV).eval()
        with torch.no_grad():
            assert bool(torch.isfinite(m(x[:128], t[:128], y[:128])[0]).all())
    assert not calls

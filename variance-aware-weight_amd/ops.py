"""Tensor-level wrappers over the C ABI (include/vaw_hip.h).  Each takes torch CUDA tensors, checks what the
kernel assumes about them (shape, dtype, contiguity) on the host, and launches on the current stream."""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import BF16, F32, AttnDesc, Epilogue, Fp8QuantJob, ReduceJob, WgradProblem, check, need_cuda, ptr, stream_ptr


def dt_of(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise L.VawError(f"unsupported activation dtype {t.dtype}")


def _f32c(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.VawError(f"expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")


# ---- diffusion objective -----------------------------------------------------------------------
def qsample(x0, noise, t, tab_a, tab_s):
    need_cuda(x0, noise, t, tab_a, tab_s)
    _f32c(x0, noise, tab_a, tab_s)
    assert noise.shape == x0.shape and t.dtype == torch.int64 and t.shape == (x0.shape[0],)
    out = torch.empty_like(x0)
    B = x0.shape[0]
    check(L.lib().vaw_qsample_fwd(ptr(x0), ptr(noise), ptr(t), ptr(tab_a), ptr(tab_s), tab_a.numel(), ptr(out), B,
                                  x0.numel() // B, stream_ptr()), "vaw_qsample_fwd")
    return out


def mix_rows(x, y, ca, cb):
    need_cuda(x, y, ca, cb)
    _f32c(x, y, ca, cb)
    assert x.shape == y.shape and ca.shape == cb.shape == (x.shape[0],)
    out = torch.empty_like(x)
    B = x.shape[0]
    check(L.lib().vaw_mix_rows(ptr(x), ptr(y), ptr(ca), ptr(cb), ptr(out), B, x.numel() // B, stream_ptr()), "vaw_mix_rows")
    return out


class _WeightedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_out, x0, noise, ca, cb, w):
        need_cuda(model_out, x0, noise, ca, cb, w)
        model_out = model_out.contiguous()
        _f32c(model_out, x0, noise, ca, cb, w)
        B = x0.shape[0]
        assert model_out.shape == x0.shape == noise.shape and ca.shape == cb.shape == w.shape == (B,)
        mse = torch.empty(B, device=x0.device, dtype=torch.float32)
        check(L.lib().vaw_wmse_fwd(ptr(model_out), ptr(x0), ptr(noise), ptr(ca), ptr(cb), ptr(w), ptr(mse), B,
                                   x0.numel() // B, stream_ptr()), "vaw_wmse_fwd")
        ctx.save_for_backward(model_out, x0, noise, ca, cb, w)
        return mse

    @staticmethod
    def backward(ctx, gmse):
        model_out, x0, noise, ca, cb, w = ctx.saved_tensors
        gmse = gmse.contiguous().float()
        dout = torch.empty_like(model_out)
        B = x0.shape[0]
        check(L.lib().vaw_wmse_bwd(ptr(model_out), ptr(x0), ptr(noise), ptr(ca), ptr(cb), ptr(w), ptr(gmse), ptr(dout),
                                   B, x0.numel() // B, stream_ptr()), "vaw_wmse_bwd")
        return dout, None, None, None, None, None


def weighted_mse(model_out, x0, noise, ca, cb, w):
    """mse[b] = w[b] * mean((ca[b]*x0 + cb[b]*noise - model_out)^2); differentiable in model_out."""
    return _WeightedMSE.apply(model_out, x0, noise, ca, cb, w)


def latent_qsample(latent, eps, noise, t, tab_a, tab_s, latent_scale, t_scale=None):
    """sample_from_latent and qsample in one launch: latent [B, 2C, H, W] (mean | std planes), eps and noise [B, C, H, W] ->
    (x0, x_t[, float(t) * t_scale]), each bitwise what the tensor operations and vaw_qsample_fwd give."""
    need_cuda(latent, eps, noise, t, tab_a, tab_s)
    _f32c(latent, eps, noise, tab_a, tab_s)
    B = latent.shape[0]
    assert latent.shape[1] % 2 == 0 and eps.shape == noise.shape == (B, latent.shape[1] // 2, *latent.shape[2:])
    assert t.dtype == torch.int64 and t.shape == (B,) and t.is_contiguous()
    x0, x_t = torch.empty_like(eps), torch.empty_like(eps)
    tf = torch.empty(B, device=eps.device, dtype=torch.float32) if t_scale is not None else None
    check(L.lib().vaw_latent_qsample(ptr(latent), ptr(eps), ptr(noise), ptr(t), ptr(tab_a), ptr(tab_s), tab_a.numel(),
                                     float(latent_scale), float(t_scale or 0.0), ptr(x0), ptr(x_t), ptr(tf), B, eps.numel() // B,
                                     stream_ptr()), "vaw_latent_qsample")
    return (x0, x_t, tf) if t_scale is not None else (x0, x_t)


class _WeightedMSEMean(torch.autograd.Function):
    """(per-sample mse [B], mean(mse) / accum) of the weighted MSE with the coefficient gather inside (vaw_wmse_fwd_t); the scalar is
    the differentiable output, and its backward hands g / (B * accum) to the kernel directly -- no ones_like / expand / div / mul."""

    @staticmethod
    def forward(ctx, model_out, x0, noise, t, ca, cb, w, accum):
        need_cuda(model_out, x0, noise, t, ca, cb, w)
        model_out = model_out.contiguous()
        _f32c(model_out, x0, noise, ca, cb, w)
        B = x0.shape[0]
        assert model_out.shape == x0.shape == noise.shape
        if t is None:
            assert ca.shape == cb.shape == w.shape == (B,)
        else:
            assert t.dtype == torch.int64 and t.shape == (B,) and t.is_contiguous() and ca.shape == cb.shape == w.shape
        mse = torch.empty(B, device=x0.device, dtype=torch.float32)
        mean = torch.empty((), device=x0.device, dtype=torch.float32)
        check(L.lib().vaw_wmse_fwd_t(ptr(model_out), ptr(x0), ptr(noise), ptr(t), ptr(ca), ptr(cb), ptr(w), ca.numel(), ptr(mse),
                                     ptr(mean), float(accum), B, x0.numel() // B, stream_ptr()), "vaw_wmse_fwd_t")
        ctx.save_for_backward(model_out, x0, noise, t, ca, cb, w)
        # 1 / (B * accum) as the two f32 divisions of the chain round it: (1 / accum) / B
        ctx.inv_count = float((torch.tensor(1.0) / float(accum)) / float(B))
        ctx.mark_non_differentiable(mse)
        ctx.set_materialize_grads(False)      # no zeros [B] for the per-sample output's absent gradient
        return mse, mean

    @staticmethod
    def backward(ctx, _gmse, gmean):
        if gmean is None:
            return (None,) * 8
        model_out, x0, noise, t, ca, cb, w = ctx.saved_tensors
        need_cuda(gmean)
        gmean = gmean.contiguous().float()
        dout = torch.empty_like(model_out)
        B = x0.shape[0]
        check(L.lib().vaw_wmse_bwd_t(ptr(model_out), ptr(x0), ptr(noise), ptr(t), ptr(ca), ptr(cb), ptr(w), ca.numel(), ptr(gmean),
                                     ctx.inv_count, ptr(dout), B, x0.numel() // B, stream_ptr()), "vaw_wmse_bwd_t")
        return dout, None, None, None, None, None, None, None


def weighted_mse_mean(model_out, x0, noise, t, ca, cb, w, accum=1):
    """(mse[b] = w * mean((ca * x0 + cb * noise - model_out)^2) per sample, detached; mean_b(mse) / accum, differentiable in model_out).
    ca / cb / w are tables gathered at t[b] inside the kernel, or per-sample vectors with t = None."""
    return _WeightedMSEMean.apply(model_out, x0, noise, t, ca, cb, w, accum)


_ones = {}


def one_like(x):
    """A resident 0-dim 1.0 on x's device: the seed gradient of a scalar loss without the ones_like fill launch of backward()."""
    t = _ones.get(x.device)
    if t is None:
        t = _ones[x.device] = torch.ones((), device=x.device, dtype=torch.float32)
    return t


class _VbTerms(torch.autograd.Function):
    """vb[b] of reference _vb_terms_bpd (gaussian_diffusion.py:775-808), one fused pass; d/d(var values) and, when the
    mean prediction is not detached (pure KL losses), d/d(mean output)."""

    @staticmethod
    def forward(ctx, mean_out, var_out, x0, x_t, coef, mean_mode, var_mode, scale):
        need_cuda(mean_out, x0, x_t, coef)
        _f32c(mean_out, x0, x_t, coef)
        B = x0.shape[0]
        assert mean_out.shape == x0.shape == x_t.shape and coef.shape == (B, 16)
        if var_out is not None:
            need_cuda(var_out)
            _f32c(var_out)
            assert var_out.shape == x0.shape
        vb = torch.empty(B, device=x0.device, dtype=torch.float32)
        check(L.lib().vaw_vb_fwd(ptr(mean_out), ptr(var_out) if var_out is not None else None, ptr(x0), ptr(x_t), ptr(coef),
                                 mean_mode, var_mode, scale, ptr(vb), B, x0.numel() // B, stream_ptr()), "vaw_vb_fwd")
        ctx.save_for_backward(mean_out, var_out, x0, x_t, coef)
        ctx.modes = (mean_mode, var_mode, scale)
        return vb

    @staticmethod
    def backward(ctx, gvb):
        mean_out, var_out, x0, x_t, coef = ctx.saved_tensors
        mean_mode, var_mode, scale = ctx.modes
        gvb = gvb.contiguous().float()
        d_mean = torch.empty_like(mean_out) if ctx.needs_input_grad[0] else None
        d_var = torch.empty_like(var_out) if (var_out is not None and ctx.needs_input_grad[1]) else None
        B = x0.shape[0]
        if d_mean is not None or d_var is not None:
            check(L.lib().vaw_vb_bwd(ptr(mean_out), ptr(var_out) if var_out is not None else None, ptr(x0), ptr(x_t), ptr(coef),
                                     mean_mode, var_mode, scale, ptr(gvb), ptr(d_mean) if d_mean is not None else None,
                                     ptr(d_var) if d_var is not None else None, B, x0.numel() // B, stream_ptr()), "vaw_vb_bwd")
        return d_mean, d_var, None, None, None, None, None, None


def vb_terms(mean_out, var_out, x0, x_t, coef, mean_mode, var_mode, scale=1.0):
    """Per-sample variational-bound term in bits/dim; see vaw_vb_fwd in include/vaw_hip.h."""
    return _VbTerms.apply(mean_out.contiguous(), None if var_out is None else var_out.contiguous(), x0, x_t, coef,
                          int(mean_mode), int(var_mode), float(scale))


def _step_outputs(kind, x, want_all):
    res = {"pred_xstart": torch.empty_like(x)}
    if kind:
        res["sample"] = torch.empty_like(x)
    if want_all:
        res["mean"], res["log_variance"] = torch.empty_like(x), torch.empty_like(x)
    return res


def _rows_in_place(ts, n):
    """The given [B, ...] tensors (None allowed) as float32 with one distance between row starts: (tensors, that distance).
    A tensor whose rows are dense but further apart than their length n (a part of a [B, 2C, H, W] or stacked [2N, ...] model
    output) is read in place; if any is laid out otherwise, or the distances differ, all are copied to contiguous."""
    def view(t):
        t = t if t.dtype == torch.float32 else t.float()
        if t.shape[0] == 1 or t.is_contiguous():
            return t.contiguous(), n
        return (t, t.stride(0)) if t[0].is_contiguous() and t.stride(0) >= n else (t.contiguous(), n)

    rows = [None if t is None else view(t) for t in ts]
    lds = {r[1] for r in rows if r is not None}
    if len(lds) > 1:
        return [None if r is None else r[0].contiguous() for r in rows], n
    return [None if r is None else r[0] for r in rows], (lds.pop() if lds else n)


def sample_step(kind, mean_out, var_out, x, noise, coef, mean_mode, var_mode, clip_denoised, eta=0.0, want_all=False):
    """One reverse-process step without guidance: kind 0 = p_mean_variance only, 1 = p_sample, 2 = ddim_sample.
    Returns {"sample", "pred_xstart"} (+ "mean", "log_variance" with want_all).  The two halves of a [B, 2C, H, W] model
    output split along dim 1 are read in place."""
    assert mean_out.shape == x.shape and coef.shape == (x.shape[0], 16) and coef.dtype == torch.float32
    return guided_sample_step(kind, mean_out, None, var_out, None, 1.0, x, noise, coef, mean_mode, var_mode, clip_denoised, eta, want_all)


def guided_sample_step(kind, mean_cond, mean_uncond, var_cond, var_uncond, guidance_scale, x, noise, coef, mean_mode, var_mode,
                       clip_denoised, eta=0.0, want_all=False):
    """One reverse-process step with classifier-free guidance fused in (vaw_guided_sample_step): per element
    m = mean_uncond + guidance_scale * (mean_cond - mean_uncond), the variance values likewise, then p_mean_variance and the
    update of `kind` (0 none, 1 p_sample, 2 ddim_sample, 3 the DDIM reverse step: no noise, no variance, no want_all).
    The four tensors are x-shaped views of the stacked [2N, 2C, H, W] model output and are read in place.  mean_uncond=None:
    the unguided step.  Returns {"sample", "pred_xstart"} (+ "mean", "log_variance" with want_all), bitwise what the three
    torch ops followed by the unguided step give."""
    need_cuda(mean_cond, mean_uncond, var_cond, var_uncond, x, noise, coef)
    x = x.contiguous().float()
    noise = None if noise is None else noise.contiguous().float()
    coef = coef.contiguous()
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    if kind == 3:
        var_mode = 0
    if var_mode == 0:
        var_cond = var_uncond = None
    if mean_uncond is None:
        var_uncond = None
    for t in (mean_cond, mean_uncond, var_cond, var_uncond):
        if t is not None and t.shape != x.shape:
            raise L.VawError(f"guided_sample_step: model output part {tuple(t.shape)} != x {tuple(x.shape)}")
    if not (coef.shape == (B, 16) and coef.dtype == torch.float32):
        raise L.VawError(f"guided_sample_step: coef {tuple(coef.shape)} {coef.dtype} is not f32 [{B}, 16]")
    if var_mode and (var_cond is None or (mean_uncond is not None and var_uncond is None)):
        raise L.VawError("guided_sample_step: a learned variance needs the variance values of every half")
    (mean_cond, mean_uncond, var_cond, var_uncond), ld = _rows_in_place((mean_cond, mean_uncond, var_cond, var_uncond), n)
    res = _step_outputs(kind, x, want_all and kind != 3)
    check(L.lib().vaw_guided_sample_step(kind, ptr(mean_cond), ptr(mean_uncond), ptr(var_cond), ptr(var_uncond), ld,
                                         float(guidance_scale), ptr(x), ptr(noise), ptr(coef), int(mean_mode), int(var_mode),
                                         1 if clip_denoised else 0, float(eta), ptr(res.get("sample")), ptr(res["pred_xstart"]),
                                         ptr(res.get("mean")), ptr(res.get("log_variance")), B, n, stream_ptr()),
          "vaw_guided_sample_step")
    return res


def cfg_combine(cond, uncond, guidance_scale):
    """uncond + guidance_scale * (cond - uncond) in one pass (vaw_cfg_combine), bitwise the three torch ops.  cond / uncond:
    f32 tensors of one shape, e.g. the two halves of the stacked [2N, ...] guided model output, read in place."""
    need_cuda(cond, uncond)
    if cond.shape != uncond.shape or cond.dtype != torch.float32 or uncond.dtype != torch.float32:
        raise L.VawError(f"cfg_combine: {tuple(cond.shape)} {cond.dtype} vs {tuple(uncond.shape)} {uncond.dtype}")
    B = cond.shape[0]
    n = cond.numel() // max(B, 1)
    (cond, uncond), ld = _rows_in_place((cond, uncond), n)
    out = torch.empty(cond.shape, device=cond.device, dtype=torch.float32)
    check(L.lib().vaw_cfg_combine(ptr(cond), ptr(uncond), ld, float(guidance_scale), ptr(out), B, n, stream_ptr()), "vaw_cfg_combine")
    return out


EDM_COLS, FLOW_COLS = L.EDM_COLS, L.FLOW_COLS
EDM_PRED = {"EPSILON": 0, "START_X": 1, "VELOCITY": 2}
FLOW_MEAN = {"START_X": 0, "EPSILON": 1, "VELOCITY": 2, "VECTOR": 3}
STEP_EULER, STEP_PREDICT, STEP_CORRECT = range(3)


def _dense(what, dtype, shape, *ts):
    for t in ts:
        if t is not None and not (t.dtype == dtype and t.shape == shape and t.is_contiguous()):
            raise L.VawError(f"{what}: expected a contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)} "
                             f"contiguous={t.is_contiguous()}")


def _table(what, coef, dtype, cols, *rows):
    if not (coef.dtype == dtype and coef.dim() == 2 and coef.shape[1] == cols and coef.is_contiguous()):
        raise L.VawError(f"{what}: the table is not a contiguous {dtype} [rows, {cols}]: {coef.dtype} {tuple(coef.shape)}")
    for r in rows:
        if not 0 <= int(r) < coef.shape[0]:
            raise L.VawError(f"{what}: row {r} outside the table of {coef.shape[0]} rows")


def _f32_parts(what, x, *ts):
    for t in ts:
        if t is not None and (t.shape != x.shape or t.dtype != torch.float32):
            raise L.VawError(f"{what}: model output part {tuple(t.shape)} {t.dtype} is not float32 {tuple(x.shape)}")


def edm_input(x, noise, coef, row, x_hat, model_in, model_in_dup=None):
    """Start of an EDM step (vaw_edm_input): x_hat = coef[row, 0] * x (+ coef[row, 1] * noise), float64, and the denoiser's
    float32 network input c_in * float(x_hat / s) into model_in (and model_in_dup, the second half of a stacked guided input).
    Bitwise the tensor operations of edm_sample / EDMDenoiser.forward.  Returns x_hat."""
    need_cuda(x, noise, coef, x_hat, model_in, model_in_dup)
    _dense("edm_input", torch.float64, x.shape, x, noise, x_hat)
    _dense("edm_input", torch.float32, x.shape, model_in, model_in_dup)
    _table("edm_input", coef, torch.float64, EDM_COLS, row)
    B = x.shape[0]
    check(L.lib().vaw_edm_input(ptr(x), ptr(noise), ptr(coef), int(row), coef.shape[0], ptr(x_hat), ptr(model_in), ptr(model_in_dup),
                                B, x.numel() // max(B, 1), stream_ptr()), "vaw_edm_input")
    return x_hat


def edm_step(kind, pred_type, cond, uncond, guidance_scale, x_hat, d_cur, coef, row, x_out=None, model_in=None, model_in_dup=None):
    """After a network evaluation of an EDM step (vaw_edm_step): kind STEP_EULER / STEP_CORRECT write and return x_out,
    STEP_PREDICT writes d_cur and the network input of the midpoint (model_in, model_in_dup) and returns d_cur.  cond / uncond:
    x-shaped float32 views of the network output (uncond=None: no guidance), read in place; pred_type: a key of EDM_PRED."""
    need_cuda(cond, uncond, x_hat, d_cur, coef, x_out, model_in, model_in_dup)
    _dense("edm_step", torch.float64, x_hat.shape, x_hat, d_cur, x_out)
    _dense("edm_step", torch.float32, x_hat.shape, model_in, model_in_dup)
    _table("edm_step", coef, torch.float64, EDM_COLS, row)
    _f32_parts("edm_step", x_hat, cond, uncond)
    B = x_hat.shape[0]
    (cond, uncond), ld = _rows_in_place((cond, uncond), x_hat.numel() // max(B, 1))
    check(L.lib().vaw_edm_step(int(kind), EDM_PRED[pred_type], ptr(cond), ptr(uncond), ld, float(guidance_scale), ptr(x_hat), ptr(d_cur),
                               ptr(coef), int(row), coef.shape[0], ptr(x_out), ptr(model_in), ptr(model_in_dup), B,
                               x_hat.numel() // max(B, 1), stream_ptr()), "vaw_edm_step")
    return d_cur if kind == STEP_PREDICT else x_out


DPM_COLS = L.DPM_COLS


def dpm_input(x, coef, row, model_in, model_in_dup=None):
    """The network input of the first evaluation of a multistep sampler (vaw_dpm_input): c_in * float32(x), c_in = coef[row, 6],
    into model_in (and model_in_dup, the second half of a stacked guided input).  Bitwise EDMDenoiser.forward's product."""
    need_cuda(x, coef, model_in, model_in_dup)
    _dense("dpm_input", torch.float64, x.shape, x)
    _dense("dpm_input", torch.float32, x.shape, model_in, model_in_dup)
    _table("dpm_input", coef, torch.float64, DPM_COLS, row)
    B = x.shape[0]
    check(L.lib().vaw_dpm_input(ptr(x), ptr(coef), int(row), coef.shape[0], ptr(model_in), ptr(model_in_dup), B, x.numel() // max(B, 1),
                                stream_ptr()), "vaw_dpm_input")
    return model_in


def dpm_step(pred_type, clip, cond, uncond, guidance_scale, x, d1, d2, noise, coef, row, x_out, d0_out, model_in=None, model_in_dup=None):
    """After the network evaluation of step `row` of a multistep sampler (vaw_dpm_step): the denoised image D0 (float32, clamped
    to [-1, 1] with clip) into d0_out, x_out = a*x + b0*D0 (+ b1*d1) (+ b2*d2) (+ c*noise) in float64 with the row's
    coefficients (x_out may be x), and the next network input into model_in (and model_in_dup).  d1 / d2: the float32 denoised
    images of the two steps before, None where the step has fewer nodes; cond / uncond, pred_type as in edm_step.  Returns x_out."""
    need_cuda(cond, uncond, x, d1, d2, noise, coef, x_out, d0_out, model_in, model_in_dup)
    _dense("dpm_step", torch.float64, x.shape, x, noise, x_out)
    _dense("dpm_step", torch.float32, x.shape, d1, d2, d0_out, model_in, model_in_dup)
    _table("dpm_step", coef, torch.float64, DPM_COLS, row)
    _f32_parts("dpm_step", x, cond, uncond)
    B = x.shape[0]
    (cond, uncond), ld = _rows_in_place((cond, uncond), x.numel() // max(B, 1))
    check(L.lib().vaw_dpm_step(EDM_PRED[pred_type], 1 if clip else 0, ptr(cond), ptr(uncond), ld, float(guidance_scale), ptr(x), ptr(d1),
                               ptr(d2), ptr(noise), ptr(coef), int(row), coef.shape[0], ptr(x_out), ptr(d0_out), ptr(model_in),
                               ptr(model_in_dup), B, x.numel() // max(B, 1), stream_ptr()), "vaw_dpm_step")
    return x_out


def flow_step(kind, sde, mean_type, cond, uncond, guidance_scale, x, noise, x_pred, f0, kick, coef, row0, row1, x_out, x_out_dup=None):
    """One step of the flow samplers after a network evaluation (vaw_flow_step), float32: see include/vaw_hip.h.  Returns x_out.
    mean_type: a key of FLOW_MEAN; cond / uncond as in edm_step."""
    need_cuda(cond, uncond, x, noise, x_pred, f0, kick, coef, x_out, x_out_dup)
    _dense("flow_step", torch.float32, x.shape, x, noise, x_pred, f0, kick, x_out, x_out_dup)
    _table("flow_step", coef, torch.float32, FLOW_COLS, row0, row1)
    _f32_parts("flow_step", x, cond, uncond)
    B = x.shape[0]
    (cond, uncond), ld = _rows_in_place((cond, uncond), x.numel() // max(B, 1))
    check(L.lib().vaw_flow_step(int(kind), 1 if sde else 0, FLOW_MEAN[mean_type], ptr(cond), ptr(uncond), ld, float(guidance_scale),
                                ptr(x), ptr(noise), ptr(x_pred), ptr(f0), ptr(kick), ptr(coef), int(row0), int(row1), coef.shape[0],
                                ptr(x_out), ptr(x_out_dup), B, x.numel() // max(B, 1), stream_ptr()), "vaw_flow_step")
    return x_out


NOISE_MODES = {"bits": L.NOISE_BITS, "uniform": L.NOISE_UNIFORM, "normal": L.NOISE_NORMAL}
NOISE_TAG_NOISE, NOISE_TAG_LABELS = L.NOISE_TAG_NOISE, L.NOISE_TAG_LABELS
_NOISE_DTYPES = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float64: L.F64}


def randn_seeded(seeds, shape_or_like, draw, *, tag=NOISE_TAG_NOISE, mode="normal", dtype=None, out=None):
    """Draw number `draw` of the per-sample streams `seeds` (vaw_randn_seeded; a device int64 [B]): a [B, ...] tensor whose row b
    is Philox4x32-10 under the key seeds[b] at the counters (block, draw, tag, 0) -- a function of (seeds[b], draw, tag, element)
    alone, whatever B, the other seeds or the history.  shape_or_like: the shape, or a tensor whose shape (and dtype, unless
    `dtype` is given) to take.  mode "normal": N(0, 1) by Box-Muller, float32 (the default), bfloat16 or float64 (the float32
    value rounded / widened); "uniform": float32 in (0, 1]; "bits": the raw words as int32.  out: an optional contiguous
    destination of that shape and dtype (any element-aligned address).  GPU only."""
    like = shape_or_like if torch.is_tensor(shape_or_like) else None
    need_cuda(seeds, like, out)
    if mode not in NOISE_MODES:
        raise L.VawError(f"randn_seeded: mode {mode!r} is not one of {tuple(NOISE_MODES)}")
    shape = tuple(like.shape) if like is not None else tuple(int(s) for s in shape_or_like)
    if dtype is None:
        dtype = torch.int32 if mode == "bits" else like.dtype if (like is not None and mode == "normal") else torch.float32
    if mode == "normal":
        if dtype not in _NOISE_DTYPES:
            raise L.VawError(f"randn_seeded: normals are float32, bfloat16 or float64, not {dtype}")
        code = _NOISE_DTYPES[dtype]
    else:
        if dtype != (torch.int32 if mode == "bits" else torch.float32):
            raise L.VawError(f"randn_seeded: mode {mode!r} writes {'int32' if mode == 'bits' else 'float32'}, not {dtype}")
        code = L.F32
    if not (seeds.dtype == torch.int64 and seeds.dim() == 1 and seeds.is_contiguous() and len(shape) >= 1 and seeds.shape[0] == shape[0]):
        raise L.VawError(f"randn_seeded: seeds {seeds.dtype} {tuple(seeds.shape)} are not a contiguous int64 [{shape[0] if shape else '?'}] "
                         f"for a draw of shape {shape}")
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=seeds.device)
    else:
        _dense("randn_seeded", dtype, shape, out)
    B = shape[0]
    check(L.lib().vaw_randn_seeded(ptr(out), code, ptr(seeds), B, out.numel() // max(B, 1), int(draw), int(tag), NOISE_MODES[mode],
                                   stream_ptr()), "vaw_randn_seeded")
    return out


RK_STAGES = L.RK_STAGES


def rk_partial_count(B, per_sample):
    """Partial sums the rk kernels write for [B, per_sample] tensors (vaw_rk_partial_count): a function of the sizes alone."""
    return int(L.lib().vaw_rk_partial_count(int(B), int(per_sample)))


def _rk_partials(what, partials, B, n):
    if not (partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= rk_partial_count(B, n)):
        raise L.VawError(f"{what}: partials is not a contiguous float64 tensor of at least {rk_partial_count(B, n)} elements: "
                         f"{partials.dtype} {tuple(partials.shape)}")


def rk_stage(stage, mean_type, cond, uncond, guidance_scale, x, x_stage, coef, row, k, slots, coeffs, h, x_out=None, x_out_dup=None,
             x_new=None, atol=0.0, rtol=0.0, partials=None):
    """The pass after the network evaluation of stage `stage` of an adaptive Runge-Kutta step from x (vaw_rk_stage, float32;
    include/vaw_hip.h): k[slots[stage]] from the network output (cond / uncond as in edm_step; cond=None: it is there
    already), then with dy = sum coeffs[s] * k[slots[s]] either the next stage's state x + h * dy into x_out (and x_out_dup)
    or, with `partials`, the partial sums of the squared error ratio (h * dy) / (atol + rtol * max(|x|, |x_new|)).  Bitwise
    the tensor composition.  k: [RK_STAGES, *x.shape]; coeffs: a sequence of at most RK_STAGES Python floats (empty: k only)."""
    need_cuda(cond, uncond, x, x_stage, coef, k, x_out, x_out_dup, x_new, partials)
    _dense("rk_stage", torch.float32, x.shape, x, x_stage, x_out, x_out_dup, x_new)
    _dense("rk_stage", torch.float32, (RK_STAGES, *x.shape), k)
    if len(slots) != RK_STAGES or len(coeffs) > RK_STAGES:
        raise L.VawError(f"rk_stage: {len(slots)} slots, {len(coeffs)} coefficients for {RK_STAGES} stages")
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    ld = n
    if cond is not None:
        _table("rk_stage", coef, torch.float32, FLOW_COLS, row)
        _f32_parts("rk_stage", x, cond, uncond)
        (cond, uncond), ld = _rows_in_place((cond, uncond), n)
    if partials is not None:
        _rk_partials("rk_stage", partials, B, n)
    check(L.lib().vaw_rk_stage(int(stage), FLOW_MEAN[mean_type], ptr(cond), ptr(uncond), ld, float(guidance_scale), ptr(x), ptr(x_stage),
                               ptr(coef) if cond is not None else 0, int(row), coef.shape[0] if cond is not None else 0, ptr(k),
                               (C.c_int * RK_STAGES)(*[int(s) for s in slots]), (C.c_float * RK_STAGES)(*[float(c) for c in coeffs]),
                               len(coeffs), float(h), ptr(x_out), ptr(x_out_dup), ptr(x_new), float(atol), float(rtol), ptr(partials),
                               0 if partials is None else partials.numel(), B, n, stream_ptr()), "vaw_rk_stage")
    return partials if partials is not None else x_out


def rk_scaled_sumsq(u, v, a, b, atol, rtol, partials):
    """Partial sums of ((u - v) / (atol + rtol * max(|a|, |b|)))^2 over float32 tensors of one shape (vaw_rk_scaled_sumsq):
    the quotient in float32, squares and sums in float64.  v=None: u alone; b=None: |a| alone.  Fold with rk_sumsq_finish."""
    need_cuda(u, v, a, b, partials)
    _dense("rk_scaled_sumsq", torch.float32, u.shape, u, v, a, b)
    B = u.shape[0]
    n = u.numel() // max(B, 1)
    _rk_partials("rk_scaled_sumsq", partials, B, n)
    check(L.lib().vaw_rk_scaled_sumsq(ptr(u), ptr(v), ptr(a), ptr(b), float(atol), float(rtol), ptr(partials), partials.numel(), B, n,
                                      stream_ptr()), "vaw_rk_scaled_sumsq")
    return partials


def rk_sumsq_finish(partials, count, out):
    """out[0] = the first `count` partial sums, folded on the device in a fixed order (vaw_rk_sumsq_finish).  out: a float64
    tensor (a one-element view of a larger one will do).  Returns out."""
    need_cuda(partials, out)
    if not (partials.dtype == out.dtype == torch.float64 and partials.is_contiguous() and 0 < count <= partials.numel() and out.numel() >= 1):
        raise L.VawError(f"rk_sumsq_finish: {count} of {partials.dtype} {tuple(partials.shape)} into {out.dtype} {tuple(out.shape)}")
    check(L.lib().vaw_rk_sumsq_finish(ptr(partials), int(count), ptr(out), stream_ptr()), "vaw_rk_sumsq_finish")
    return out


FLOW_LOGP_COLS = L.FLOW_LOGP_COLS


def flow_logp_stage(stage, out, g, eps, x, x_stage, coef, row, k, d, coeffs, h, x_out=None, delta=None, partials=None):
    """The pass after the network evaluation and the vector-Jacobian product of stage `stage` of a Runge-Kutta step of the
    log-likelihood integration (vaw_flow_logp_stage; include/vaw_hip.h): k[stage] = A * x_stage + B * out from coef[row]
    (float32, bitwise the tensor composition), d[stage] = A * n + B * sum(eps * g) per row in float64, and with `coeffs`
    x + h * sum coeffs[s] * k[s] into x_out; with `delta` (the last stage) delta += h * sum coeffs[s] * d[s] in float64.
    out: the x-shaped float32 view of the network output, read in place; k: [RK_STAGES, *x.shape] float32; d: [RK_STAGES, B]
    float64; coeffs: at most RK_STAGES Python floats; partials: rk_partial_count(B, per_sample) float64 (rows over 1024)."""
    need_cuda(out, g, eps, x, x_stage, coef, k, d, x_out, delta, partials)
    _dense("flow_logp_stage", torch.float32, x.shape, x, x_stage, g, eps, x_out)
    _dense("flow_logp_stage", torch.float32, (RK_STAGES, *x.shape), k)
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    _dense("flow_logp_stage", torch.float64, (RK_STAGES, B), d)
    _dense("flow_logp_stage", torch.float64, (B,), delta)
    _table("flow_logp_stage", coef, torch.float32, FLOW_LOGP_COLS, row)
    _f32_parts("flow_logp_stage", x, out)
    if len(coeffs) > RK_STAGES or (len(coeffs) > 0) != (x_out is not None):
        raise L.VawError(f"flow_logp_stage: {len(coeffs)} coefficients for {RK_STAGES} stages, x_out {'given' if x_out is not None else 'missing'}")
    if x_out is not None and any(x_out.data_ptr() == t.data_ptr() for t in (x, x_stage, g, eps) if t is not None):
        raise L.VawError("flow_logp_stage: x_out overlaps an input")
    if partials is not None:
        _rk_partials("flow_logp_stage", partials, B, n)
    (out,), ld = _rows_in_place((out,), n)
    check(L.lib().vaw_flow_logp_stage(int(stage), ptr(out), ld, ptr(g), ptr(eps), ptr(x), ptr(x_stage), ptr(coef), int(row), coef.shape[0],
                                      ptr(k), ptr(d), (C.c_double * RK_STAGES)(*[float(c) for c in coeffs]), len(coeffs), float(h),
                                      ptr(x_out), ptr(delta), ptr(partials), 0 if partials is None else partials.numel(), B, n,
                                      stream_ptr()), "vaw_flow_logp_stage")
    return x_out


def flow_logp_prior(z, partials=None):
    """log N(z; 0, I) per row, float64 [B] (vaw_flow_logp_prior): -1/2 sum z^2 - (n / 2) ln 2 pi with squares and sums in
    float64 in a fixed order.  partials as in flow_logp_stage (allocated when a row needs them and none is given)."""
    need_cuda(z, partials)
    _f32c(z)
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    if partials is None and n > 1024:
        partials = torch.empty(rk_partial_count(B, n), dtype=torch.float64, device=z.device)
    if partials is not None:
        _rk_partials("flow_logp_prior", partials, B, n)
    logp = torch.empty(B, dtype=torch.float64, device=z.device)
    check(L.lib().vaw_flow_logp_prior(ptr(z), ptr(logp), ptr(partials), 0 if partials is None else partials.numel(), B, n, stream_ptr()),
          "vaw_flow_logp_prior")
    return logp


def finish_images(samples, out=None):
    """[B, C, H, W] f32 / f64 samples in [-1, 1] -> [B, H, W, C] uint8 (vaw_finish_images): bitwise
    ((x + 1) * 127.5).clamp(0, 255).to(uint8).permute(0, 2, 3, 1).contiguous() for finite x; NaN writes 0.
    out: an optional contiguous uint8 [B, H, W, C] destination (any byte alignment)."""
    need_cuda(samples, out)
    if samples.dim() != 4 or samples.dtype not in (torch.float32, torch.float64):
        raise L.VawError(f"finish_images: expected a [B, C, H, W] float32 / float64 tensor, got {tuple(samples.shape)} {samples.dtype}")
    samples = samples.contiguous()
    B, Cn, H, W = samples.shape
    if out is None:
        out = torch.empty((B, H, W, Cn), device=samples.device, dtype=torch.uint8)
    elif not (out.dtype == torch.uint8 and out.shape == (B, H, W, Cn) and out.is_contiguous()):
        raise L.VawError(f"finish_images: destination {tuple(out.shape)} {out.dtype} is not a contiguous uint8 {(B, H, W, Cn)}")
    check(L.lib().vaw_finish_images(ptr(samples), 1 if samples.dtype == torch.float64 else 0, ptr(out), B, Cn, H, W, stream_ptr()),
          "vaw_finish_images")
    return out


def bpd_terms(mean_out, var_out, x0, x_t, noise, coef, mean_mode, var_mode, clip_denoised, out=None, col=0, group=None):
    """The three per-sample scalars of one calc_bpd_loop timestep (vaw_bpd_terms): returns (vb, xstart_mse, mse).
    out=None: three new [B] vectors.  Otherwise out = three f32 [N, T] tensors of equal strides with unit column stride,
    group = N and B = K*N stacked rows (K timesteps of the N samples): row b fills out[.][b % N, col + b // N]."""
    need_cuda(mean_out, var_out, x0, x_t, noise, coef)
    _f32c(x0, x_t, noise, coef)
    B = x0.shape[0]
    n = x0.numel() // max(B, 1)
    if not (mean_out.shape == x0.shape == x_t.shape == noise.shape and coef.shape == (B, 16)):
        raise L.VawError(f"bpd_terms: shapes {tuple(mean_out.shape)} {tuple(x0.shape)} {tuple(x_t.shape)} {tuple(noise.shape)} "
                         f"coef {tuple(coef.shape)} do not agree")
    if var_out is not None and var_out.shape != x0.shape:
        raise L.VawError(f"bpd_terms: var_out shape {tuple(var_out.shape)} != {tuple(x0.shape)}")
    (mean_out, var_out), ld = _rows_in_place((mean_out, var_out), n)
    if out is None:
        res = tuple(torch.empty(B, device=x0.device, dtype=torch.float32) for _ in range(3))
        ptrs, out_ld, group = [ptr(r) for r in res], 1, B
    else:
        res = tuple(out)
        group = B if group is None else int(group)
        k = B // group if group > 0 else 0
        for r in res:
            need_cuda(r)
            if not (r.dtype == torch.float32 and r.dim() == 2 and r.shape[0] == group and r.stride(1) == 1 and
                    r.stride(0) == res[0].stride(0) and r.stride(0) >= r.shape[1] and group * k == B and
                    0 <= col and col + k <= r.shape[1]):
                raise L.VawError(f"bpd_terms: output {tuple(r.shape)} strides {r.stride()} cannot take {B} rows in groups of "
                                 f"{group} from column {col}")
        ptrs, out_ld = [r.data_ptr() + 4 * col for r in res], res[0].stride(0)
    check(L.lib().vaw_bpd_terms(ptr(mean_out), ptr(var_out), ld, ptr(x0), ptr(x_t), ptr(noise), ptr(coef), int(mean_mode),
                                int(var_mode), 1 if clip_denoised else 0, ptrs[0], ptrs[1], ptrs[2], out_ld, group, B, n,
                                stream_ptr()), "vaw_bpd_terms")
    return res


def prior_bpd(x0, sqrt_abar_last, log_one_minus_abar_last):
    """KL(q(x_T | x_0) || N(0, I)) in bits/dim per sample (vaw_prior_bpd)."""
    need_cuda(x0)
    _f32c(x0)
    B = x0.shape[0]
    out = torch.empty(B, device=x0.device, dtype=torch.float32)
    check(L.lib().vaw_prior_bpd(ptr(x0), float(sqrt_abar_last), float(log_one_minus_abar_last), ptr(out), B,
                                x0.numel() // max(B, 1), stream_ptr()), "vaw_prior_bpd")
    return out


def ddim_reverse_step(mean_out, x, coef, clip_denoised):
    """One step of the DDIM ODE towards noise (kind 3 of vaw_guided_sample_step, eta = 0): {"sample", "pred_xstart"}."""
    if not (mean_out.shape == x.shape and coef.shape == (x.shape[0], 16) and coef.dtype == torch.float32):
        raise L.VawError(f"ddim_reverse_step: shapes {tuple(mean_out.shape)} {tuple(x.shape)} coef {tuple(coef.shape)} do not agree")
    return guided_sample_step(3, mean_out, None, None, None, 1.0, x, None, coef, 0, 0, clip_denoised)


# ---- dense -------------------------------------------------------------------------------------
def epilogue(*, bias=None, act=0, aux_in=None, aux_out=None, gate=None, gate_ld=0, resid=None, rowadd=None, rows_per_batch=0, alpha=1.0,
             beta=0.0, out_f32=False, colsum_out=None, colsum_beta=0.0, resid_is_act=False, rowsum_a_out=None, rowsum_a_beta=0.0,
             colsum_partial=None, colsum_partial_out=16):
    """vaw_epilogue from keywords named as its fields (addresses as integers, 0 / None = NULL): alpha = 1, everything else zero or
    null; any other keyword is a TypeError.  Every launch and its *_plan twin build theirs here, so a plan sees its launch's epilogue.
    colsum_partial = a ColsumPartial (its buffer and its host row count: in the capacity, out the rows written) or, for a plan, a
    bare row capacity, which stands at the address colsum_partial_out (any non-zero one serves)."""
    e = Epilogue(bias=bias or None, act=act, aux_in=aux_in or None, aux_out=aux_out or None, gate=gate or None, gate_ld=gate_ld,
                 resid=resid or None, rowadd=rowadd or None, rows_per_batch=rows_per_batch, alpha=alpha, beta=beta,
                 out_f32=1 if out_f32 else 0, colsum_out=colsum_out or None, colsum_beta=colsum_beta,
                 resid_is_act=1 if resid_is_act else 0, rowsum_a_out=rowsum_a_out or None, rowsum_a_beta=rowsum_a_beta)
    if colsum_partial is not None:
        if isinstance(colsum_partial, ColsumPartial):
            rows, colsum_partial_out = colsum_partial.rows, colsum_partial.buf.data_ptr()
            rows.value = colsum_partial.buf.shape[0]
        else:
            rows = C.c_int64(colsum_partial)
        e.colsum_partial_out, e.colsum_rows_out, e.rows = colsum_partial_out, C.pointer(rows), rows     # (e.rows keeps the count alive)
    return e


def _trace_open():
    """(GemmTrace that listens, e0, e1) with e0 recorded on the launch stream -- the caller launches, records e1, adds its row -- or Nones."""
    tr = gemm_trace
    if tr is None:
        return None, None, None
    e0, e1 = tr.events()
    e0.record()
    return tr, e0, e1


def gemm(dt, a_kmajor, b_kmajor, M, N, K, A, lda, B, ldb, Cp, ldc, *, bias=None, act=0, aux_in=None, aux_out=None,
         gate=None, gate_ld=0, resid=None, rowadd=None, rows_per_batch=0, alpha=1.0, beta=0.0, out_f32=False,
         colsum_out=None, colsum_beta=0.0, resid_is_act=False, rowsum_a_out=None, rowsum_a_beta=0.0, colsum_partial=None):
    """Raw-pointer GEMM; A, B, Cp, bias... are integers (device addresses).  See vaw_gemm in the header.
    colsum_partial = ColsumPartial: the column sums of C stay as partial rows in its buffer (folded later, many at once)."""
    e = epilogue(bias=bias, act=act, aux_in=aux_in, aux_out=aux_out, gate=gate, gate_ld=gate_ld, resid=resid, rowadd=rowadd,
                 rows_per_batch=rows_per_batch, alpha=alpha, beta=beta, out_f32=out_f32, colsum_out=colsum_out, colsum_beta=colsum_beta,
                 resid_is_act=resid_is_act, rowsum_a_out=rowsum_a_out, rowsum_a_beta=rowsum_a_beta, colsum_partial=colsum_partial)
    tr, e0, e1 = _trace_open()
    ws_ptr, ws_n = 0, 0
    if colsum_out or colsum_partial is not None or rowsum_a_out or (beta_or_plain(bias, act, aux_out, gate, resid, rowadd) and K >= 2048):     # may run split-K
        ws = scratch_f32(torch.device("cuda", torch.cuda.current_device()), 0)
        ws_ptr, ws_n = ws.data_ptr(), ws.numel()
    check(L.lib().vaw_gemm(dt, 1 if a_kmajor else 0, 1 if b_kmajor else 0, M, N, K, A, lda, B, ldb, Cp, ldc,
                           C.byref(e), ws_ptr, ws_n, stream_ptr()), "vaw_gemm")
    if tr is not None:
        e1.record()
        es = 2 if dt == BF16 else 4
        nb = es * (M * K + N * K) + M * N * ((4 if (out_f32 or dt == F32) else 2) + (es if aux_out else 0) + (es if aux_in else 0) +
                                             ((es if resid_is_act else 4) if resid else 0) + (4 if (beta and out_f32) else 0))
        tr.add(L.lib().vaw_gemm_uses_bf16_mfma(dt, M, N, K, A, lda, B, ldb), bool(a_kmajor), bool(b_kmajor), M, N, K, e0, e1, float(nb))


def default_gemm_knobs(**kw):
    """vaw_gemm_knobs with every knob at its default and 256 CUs (no environment), then the given fields."""
    k = L.GemmKnobs()
    L.lib().vaw_gemm_default_knobs(C.byref(k))
    for name, v in kw.items():
        setattr(k, name, v)
    return k


def gemm_plan(dt, a_kmajor, b_kmajor, M, N, K, A, lda, B, ldb, Cp, ldc, *, workspace_floats=0, knobs=None, colsum_partial_rows=None,
              check_status=True, **epi):
    """The launch vaw_gemm makes for this call (vaw_gemm_plan: host arithmetic, no GPU).  Arguments as for gemm(), the addresses used
    for null-ness and alignment only; colsum_partial_rows = capacity of a colsum_partial buffer (any non-zero address stands for
    it); knobs = None: the process's own, else a GemmKnobs (default_gemm_knobs).  check_status = False returns the plan of a
    refused call (status != 0) instead of raising."""
    e = epilogue(colsum_partial=colsum_partial_rows, **epi)
    p = L.GemmLaunch()
    rc = L.lib().vaw_gemm_plan(dt, 1 if a_kmajor else 0, 1 if b_kmajor else 0, M, N, K, lda, ldb, ldc, A, B, Cp, C.byref(e),
                               workspace_floats, C.byref(knobs) if knobs is not None else None, C.byref(p))
    if check_status:
        check(rc, "vaw_gemm_plan")
    return p


# ---- fp8 operands ------------------------------------------------------------------------------------
def fp8_quantize(src_dt, src, R, C_, ld, q, qt, scale, fmt=L.FP8, device=None):
    """Raw-pointer vaw_fp8_quantize: src [R][C] (row stride ld) -> q [R][C] bytes, qt [C][R] bytes (0 = not wanted), scale."""
    ws = scratch_f32(device or torch.device("cuda", torch.cuda.current_device()), 0)
    check(L.lib().vaw_fp8_quantize(src_dt, fmt, src, R, C_, ld, q, C_, qt or None, R, scale, ws.data_ptr(), ws.numel(), stream_ptr()),
          "vaw_fp8_quantize")


FP8_MAX = {L.FP8: 448.0, L.BF8: 57344.0}


def fp8_states(formats, device, margin=2.0):
    """[n][4] f32 scaling states {scale, running amax, FMAX / margin, 0} for delayed scaling (vaw_fp8_quantize_delayed /
    vaw_fp8_scale_update), one row per tensor format in `formats`."""
    st = torch.zeros(len(formats), 4)
    st[:, 0] = 1.0
    st[:, 2] = torch.tensor([FP8_MAX[f] / margin for f in formats])
    return st.to(device)


def fp8_scale_update(states, finite=False):
    """finite (runs behind the step guard): a running max that is not finite keeps the scale in use (vaw_fp8_scale_update_finite)."""
    if finite:
        check(L.lib().vaw_fp8_scale_update_finite(states.data_ptr(), states.shape[0], stream_ptr()), "vaw_fp8_scale_update_finite")
        return
    check(L.lib().vaw_fp8_scale_update(states.data_ptr(), states.shape[0], stream_ptr()), "vaw_fp8_scale_update")


class Fp8:
    """An fp8 copy of a 2-D operand: q [R][C] bytes, optionally qt [C][R] (the transposed copy the k-major-only fp8 GEMMs read
    for the other contraction), and the device scalar `scale` that turns the bytes back into values.  fmt: FP8 (e4m3) | BF8 (e5m2).
    plain=False keeps only the transposed copy (the row-major bytes go to the buffer `q_scratch` hands out).  state: a row of
    fp8_states() shared with the once-per-step scale update (delayed scaling); without one the object owns a private row."""

    def __init__(self, R, C_, device, transposed=True, plain=True, fmt=L.FP8, state=None):
        self.R, self.C, self.fmt, self.device = int(R), int(C_), fmt, device
        self.q = torch.empty(R, C_, device=device, dtype=torch.uint8) if plain else None
        self.qt = torch.empty(C_, R, device=device, dtype=torch.uint8) if transposed else None
        self.state = state if state is not None else fp8_states([fmt], device)[0]
        self.scale = self.state[0:1]

    def quantize(self, src, ld=None, src_dt=None, delayed=False):
        """src: f32 / bf16 tensor holding R x C values with row stride ld (default C), or a device address with src_dt.
        delayed=False: scale = amax / FMAX taken from src first (two passes); True: the scale already in the state."""
        if isinstance(src, torch.Tensor):
            need_cuda(src)
            src_dt, src = dt_of(src), src.data_ptr()
        q = self.q if self.q is not None else q_scratch(self.R * self.C, self.device)
        if delayed:
            check(L.lib().vaw_fp8_quantize_delayed(src_dt, self.fmt, src, self.R, self.C, ld or self.C, q.data_ptr(), self.C, ptr(self.qt),
                                                   self.R, self.state.data_ptr(), stream_ptr()), "vaw_fp8_quantize_delayed")
        else:
            fp8_quantize(src_dt, src, self.R, self.C, ld or self.C, q.data_ptr(), ptr(self.qt), self.scale.data_ptr(), self.fmt, self.device)
            # leave this pass's max |x| in the running-max slot too: the first vaw_fp8_scale_update after a just-in-time pass then
            # yields amax * margin / FMAX like every later one (otherwise the first delayed step would run without headroom)
            torch.mul(self.state[0:1], FP8_MAX[self.fmt], out=self.state[1:2])
        self.last_q = q.data_ptr()
        return self

    def epilogue_target(self, pool=1):
        """Row-major byte buffer a producing kernel may write this tensor's fp8 form into (gemm_fp8(out_fp8=self),
        ln_modulate_fwd_fp8, gate_bwd_fp8); finish with transpose_from_q().  Pools keep a GEMM's fp8 input (pool 0: quantiser
        outputs, pool 2: row-kernel outputs) apart from the fp8 output its epilogue writes (pool 1)."""
        q = self.q if self.q is not None else q_scratch(self.R * self.C, self.device, pool=pool)
        self.last_q = q.data_ptr()
        return self.last_q

    def transpose_from_q(self):
        check(L.lib().vaw_fp8_transpose(self.last_q, self.R, self.C, self.C, self.qt.data_ptr(), self.R, stream_ptr()), "vaw_fp8_transpose")
        return self

    def dequant(self):
        return self.q.view(torch.float8_e5m2 if self.fmt == L.BF8 else torch.float8_e4m3fn).float() * self.scale


class TableGroup:
    """Base of the "one launch for many problems" groups: the host table of `rows` (records of type `rec`), its device copy `desc`
    and the upload flag.  The addresses in a table stay put while its group lives, so only the group's first launch uploads."""

    def __init__(self, rec, rows, desc_bytes, device):
        self.n, self.uploaded = len(rows), False
        self.table = (rec * self.n)(*rows)
        self.desc = torch.empty(desc_bytes(self.n), device=device, dtype=torch.uint8)

    def _call(self, name, *pre, post=()):        # lib.<name>(*pre, desc, upload, *post, stream): upload = 1 until one call succeeded
        check(getattr(L.lib(), name)(*pre, self.desc.data_ptr(), 0 if self.uploaded else 1, *post, stream_ptr()), name)
        self.uploaded = True


class GroupCache(collections.OrderedDict):
    """key -> launch group, at most `bound` of them: get() builds a missing one and drops the least recently used beyond the bound
    (torch frees its device table like any tensor, in stream order).  A model's copy (EMA) has other addresses: it starts empty."""

    def __init__(self, bound):
        super().__init__()
        self.bound, self.hits, self.misses = int(bound), 0, 0

    def get(self, key, build):
        if key in self:
            self.hits += 1
            self.move_to_end(key)
            return self[key]
        self.misses += 1
        grp = self[key] = build()
        while len(self) > self.bound:
            self.popitem(last=False)
        return grp

    def __deepcopy__(self, memo):
        return GroupCache(self.bound)


class Fp8QuantGroup(TableGroup):
    """Delayed-scaling e4m3 quantisation of many f32 tensors (src address, Fp8 with q and qt) in ONE vaw_fp8_quantize_delayed_batched."""

    def __init__(self, pairs, device):
        jobs = [Fp8QuantJob(src, f.q.data_ptr(), ptr(f.qt), f.state.data_ptr(), f.R, f.C, f.C, f.C, f.R) for src, f in pairs]
        super().__init__(Fp8QuantJob, jobs, L.lib().vaw_fp8_quantize_batched_desc_bytes, device)
        self.fp8s = [f for _, f in pairs]

    def launch(self):
        self._call("vaw_fp8_quantize_delayed_batched", self.n, self.table)
        for f in self.fp8s:
            f.last_q = f.q.data_ptr()


_q_scratch = {}


def q_scratch(n, device, pool=0):
    """Grow-only byte scratch for row-major fp8 copies that only the very next GEMM reads (pool 0: quantiser outputs, pool 1:
    tensors a GEMM epilogue writes as fp8 while its input operand sits in pool 0)."""
    t = _q_scratch.get((device, pool))
    if t is None or t.numel() < n:
        t = _q_scratch[(device, pool)] = torch.empty(n, device=device, dtype=torch.uint8)
    return t


def gemm_fp8(M, N, K, A, lda, scale_a, B, ldb, scale_b, Cp, ldc, *, a_format=L.FP8, bias=None, act=0, aux_in=None, aux_out=None,
             gate=None, gate_ld=0, resid=None, rows_per_batch=0, alpha=1.0, out_f32=False, colsum_out=None, colsum_beta=0.0,
             out_fp8=None, colsum_partial=None):
    """Raw-pointer fp8 GEMM (vaw_gemm_fp8): A [M][K] bytes of a_format, B [N][K] e4m3 bytes; scale_a / scale_b device scalars.
    out_fp8 = an Fp8 whose delayed-scaling state is current: C (= its row-major bytes) is written as fp8 by the epilogue."""
    # (the fp8 launch has no rowadd, beta, resid_is_act or rowsum_a_out keyword: they stay null / zero)
    e = epilogue(bias=bias, act=act, aux_in=aux_in, aux_out=aux_out, gate=gate, gate_ld=gate_ld, resid=resid, rows_per_batch=rows_per_batch,
                 alpha=alpha, out_f32=out_f32, colsum_out=colsum_out, colsum_beta=colsum_beta, colsum_partial=colsum_partial)
    tr, e0, e1 = _trace_open()
    ws_ptr, ws_n = 0, 0
    if colsum_out:
        ws = scratch_f32(torch.device("cuda", torch.cuda.current_device()), 0)
        ws_ptr, ws_n = ws.data_ptr(), ws.numel()
    check(L.lib().vaw_gemm_fp8(a_format, M, N, K, A, lda, scale_a, B, ldb, scale_b, Cp, ldc, C.byref(e),
                               out_fp8.state.data_ptr() if out_fp8 is not None else None, out_fp8.fmt if out_fp8 is not None else 0,
                               ws_ptr, ws_n, stream_ptr()), "vaw_gemm_fp8")
    if tr is not None:
        e1.record()
        nb = M * K + N * K + M * N * ((4 if out_f32 else 1 if out_fp8 is not None else 2) + (2 if aux_out else 0) + (2 if aux_in else 0) +
                                      (4 if resid else 0))
        tr.add(2, True, a_format == L.FP8, M, N, K, e0, e1, float(nb))


def gemm_fp8_plan(M, N, K, A, lda, scale_a, B, ldb, scale_b, Cp, ldc, *, a_format=L.FP8, workspace=16, workspace_floats=0, cus=0,
                  colsum_partial_rows=None, out_fp8_state=0, out_fp8_format=L.FP8, check_status=True, **epi):
    """The launch vaw_gemm_fp8 makes for this call (vaw_gemm_fp8_plan: host arithmetic, no GPU).  Arguments as for gemm_fp8(), the
    addresses used for null-ness and alignment only; out_fp8_state = address of the delayed-scaling state of an fp8 output (0: none)
    and out_fp8_format its format; colsum_partial_rows = capacity of a colsum_partial buffer (any non-zero address stands for it);
    workspace_floats = 0 stands for no workspace; cus = 0: the CUs the process may use now, else a stated count.
    check_status = False returns the plan of a refused call (status != 0) instead of raising."""
    # (what gemm_fp8 has no keyword for -- rowadd, beta, ... -- is passed on, so that the plan can be asked why it refuses them)
    e = epilogue(colsum_partial=colsum_partial_rows, **epi)
    p = L.GemmFp8Launch()
    rc = L.lib().vaw_gemm_fp8_plan(a_format, M, N, K, A, lda, scale_a, B, ldb, scale_b, Cp, ldc, C.byref(e), out_fp8_state, out_fp8_format,
                                   workspace if workspace_floats > 0 else 0, workspace_floats, cus, C.byref(p))
    if check_status:
        check(rc, "vaw_gemm_fp8_plan")
    return p


class WgradGroup(TableGroup):
    """The weight gradients dW_p (+)= dy_p^T x_p of many Linear layers as ONE launch (vaw_wgrad_grouped).  `problems` is a list of
    (dy_addr, x_addr, dw_addr, M, N, ld_dy, ld_x, ld_dw)."""

    def __init__(self, problems, K, device):
        super().__init__(WgradProblem, [WgradProblem(*p) for p in problems], L.lib().vaw_wgrad_grouped_desc_bytes, device)
        self.K, self.device = int(K), device
        self.flop = sum(2.0 * p[3] * p[4] * K for p in problems)

    def launch(self, dt, beta):
        ws = scratch_f32(self.device, 0)
        tr, e0, e1 = _trace_open()
        self._call("vaw_wgrad_grouped", dt, self.n, self.table, self.K, float(beta), post=(ws.data_ptr(), ws.numel()))
        if tr is not None:
            e1.record()
            es = 1 if dt in (L.FP8, L.BF8) else 2
            tr.add_flop(2 if dt in (L.FP8, L.BF8) else 1, False, False, self.flop, e0, e1,
                        float(sum(es * (p.M + p.N) * self.K + 4 * p.M * p.N * (2 if beta else 1) for p in self.table)))


def wgrad_engine(mode):
    """Engine of the bf16 256-column launches of vaw_wgrad_grouped from now on (vaw_debug_wgrad_engine): -1 by shape, 0 the 8-wave
    kernel, 1 the 4-wave kernel.  Both give the same bits; for tests and A/B measurements."""
    L.lib().vaw_debug_wgrad_engine(int(mode))


def beta_or_plain(bias, act, aux_out, gate, resid, rowadd):
    """True when the epilogue is alpha/beta only: the launches that may run split-K."""
    return not (bias or act or aux_out or gate or resid or rowadd)


def conv3x3(dt, mode, act, act2, w, out, B, H, W, Ci, Co, *, bias=None, resid=None, resid_is_act=True, beta=0.0,
            colsum_out=None, colsum_beta=0.0, rowsum_a_out=None, rowsum_a_beta=0.0):
    """Implicit-GEMM conv3x3 (vaw_conv3x3).  Returns False -- nothing launched -- when the shape needs the explicit
    im2col + GEMM path.  mode 0 forward, 1 input gradient, 2 weight gradient (f32 out, beta accumulates)."""
    # (act stays 0 in the struct: the convolution's activations are operands of the call; the weight gradient is f32)
    e = epilogue(bias=bias, resid=resid, resid_is_act=resid_is_act, beta=beta, out_f32=mode == 2, colsum_out=colsum_out, colsum_beta=colsum_beta,
                 rowsum_a_out=rowsum_a_out, rowsum_a_beta=rowsum_a_beta)
    ws = scratch_f32(torch.device("cuda", torch.cuda.current_device()), 0)
    tr, e0, e1 = _trace_open()
    rc = L.lib().vaw_conv3x3(dt, mode, act, act2 or None, w, out, B, H, W, Ci, Co, C.byref(e), ws.data_ptr(), ws.numel(), stream_ptr())
    if rc == -3:
        if dt == L.BF16:       # the f32 parity mode always takes the explicit path; in bf16 it is a performance cliff worth a word
            key = ("conv3x3", ("fwd", "dgrad", "wgrad")[mode], B, H, W, Ci, Co)
            fallbacks[key] = fallbacks.get(key, 0) + 1
            if fallbacks[key] == 1:
                import warnings
                warnings.warn(f"vaw_amd: conv3x3 {key[1]} [B={B}, {H}x{W}, Ci={Ci}, Co={Co}] is not covered by the implicit-GEMM kernels "
                              "(channel counts off the 64 / 8 grid?): falling back to im2col + GEMM; counts in vaw_amd.ops.fallbacks",
                              RuntimeWarning, stacklevel=3)
        return False
    check(rc, "vaw_conv3x3")
    if tr is not None:
        e1.record()
        M = B * H * W
        nb = 2 * M * (Ci + Co) + (2 if mode != 2 else 4 * (2 if beta else 1)) * 9 * Ci * Co + ((2 * M * Co) if (mode == 0 and resid) else 0)
        tr.add(1, mode != 2, mode == 0, *((M, Co, 9 * Ci) if mode == 0 else (M, Ci, 9 * Co) if mode == 1 else (Co, 9 * Ci, M)), e0, e1, float(nb), tag=f"conv{H}x{W}")
    return True


def conv3x3_plan(dt, mode, act, act2, w, out, B, H, W, Ci, Co, *, workspace=16, workspace_floats=0, knobs=None, cus=0, check_status=True,
                 **epi):
    """The launch vaw_conv3x3 makes for this call (vaw_conv3x3_plan: host arithmetic, no GPU).  Arguments and epilogue keywords as
    for conv3x3(), the addresses used for null-ness and alignment only; workspace_floats = 0 stands for no workspace; knobs = None:
    the process's own, else a GemmKnobs (default_gemm_knobs); cus = 0: the CUs the process may use now (or the knobs' count).
    check_status = False returns the plan of a refused call (status -1 invalid, -3 the explicit path) instead of raising."""
    # (as conv3x3 forces them: residual in the act dtype by default, mode 2 in f32; aux_in, rows_per_batch and alpha are not the caller's)
    e = epilogue(**dict(epi, resid_is_act=epi.get("resid_is_act", True), out_f32=mode == 2 or epi.get("out_f32"), aux_in=None, rows_per_batch=0, alpha=1.0))
    p = L.Conv3x3Launch()
    rc = L.lib().vaw_conv3x3_plan(dt, mode, act or 0, act2 or 0, w or 0, out or 0, B, H, W, Ci, Co, C.byref(e),
                                  workspace if workspace_floats > 0 else 0, workspace_floats, C.byref(knobs) if knobs is not None else None,
                                  cus, C.byref(p))
    if check_status:
        check(rc, "vaw_conv3x3_plan")
    return p


fallbacks = {}       # (op, variant, shape...) -> times a bf16 launch left the fast kernels for the explicit path


class GemmTrace:
    """Measurement aid (bench.py): brackets every GEMM launch with HIP events on the launch stream."""

    def __init__(self):
        self.rows = []

    def events(self):
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def add(self, mfma, ak, bk, M, N, K, e0, e1, nbytes=0.0, tag="gemm"):
        self.rows.append((mfma, ak, bk, 2.0 * M * N * K, e0, e1, nbytes, (tag, int(M), int(N), int(K))))

    def add_flop(self, mfma, ak, bk, flop, e0, e1, nbytes=0.0):
        self.rows.append((mfma, ak, bk, flop, e0, e1, nbytes, None))

    @staticmethod
    def _name(mfma, ak, bk):
        return ("fp8_mfma" if mfma == 2 else "bf16_mfma" if mfma else "generic_f32mfma") + ("/fwd" if ak and bk else "/dgrad" if ak else "/wgrad")

    def by_shape(self):
        """-> [(variant, (M, N, K) or None, launches, ms, flop)] sorted by time, after a device synchronize (bench.py --shape-table)."""
        acc = {}
        for mfma, ak, bk, flop, e0, e1, nbytes, shape in self.rows:
            d = acc.setdefault((self._name(mfma, ak, bk), shape), [0, 0.0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
            d[2] += flop
        return sorted(((k[0], k[1], v[0], v[1], v[2]) for k, v in acc.items()), key=lambda r: -r[3])

    def summarize(self):
        """-> {variant: {launches, flop, ms}} after a device synchronize."""
        out = {}
        for mfma, ak, bk, flop, e0, e1, nbytes, _shape in self.rows:
            name = self._name(mfma, ak, bk)
            d = out.setdefault(name, {"launches": 0, "flop": 0.0, "ms": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["flop"] += flop
            d["bytes"] += nbytes          # algorithmic: every operand and result once
            d["ms"] += e0.elapsed_time(e1)
        return out


gemm_trace = None


def gemm_t(A, B, *, a_kmajor=True, b_kmajor=True, out_dtype=None, bias=None, act=0, aux_in=None, want_aux=False,
           gate=None, resid=None, rowadd=None, rows_per_batch=0, alpha=1.0, beta=0.0, out=None, colsum_out=None,
           colsum_beta=0.0, rowsum_a_out=None, rowsum_a_beta=0.0):
    """Tensor-level GEMM for tests and small call sites: A, B 2-D contiguous, same dtype."""
    need_cuda(A, B)
    assert A.dim() == 2 and B.dim() == 2 and A.is_contiguous() and B.is_contiguous() and A.dtype == B.dtype
    dt = dt_of(A)
    M, K = (A.shape if a_kmajor else A.shape[::-1])
    N, Kb = (B.shape if b_kmajor else B.shape[::-1])
    assert K == Kb, (A.shape, B.shape, a_kmajor, b_kmajor)
    out_dtype = out_dtype or A.dtype
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=out_dtype)
    aux = torch.empty(M, N, device=A.device, dtype=A.dtype) if want_aux else None
    _f32c(bias, gate, resid, rowadd)
    gemm(dt, a_kmajor, b_kmajor, M, N, K, ptr(A), A.shape[1], ptr(B), B.shape[1], ptr(out), N, bias=ptr(bias), act=act,
         aux_in=ptr(aux_in), aux_out=ptr(aux), gate=ptr(gate), gate_ld=(gate.shape[-1] if gate is not None else 0),
         resid=ptr(resid), rowadd=ptr(rowadd), rows_per_batch=rows_per_batch, alpha=alpha, beta=beta,
         out_f32=(out.dtype == torch.float32), colsum_out=ptr(colsum_out), colsum_beta=colsum_beta,
         rowsum_a_out=ptr(rowsum_a_out), rowsum_a_beta=rowsum_a_beta)
    return (out, aux) if want_aux else out


_scratch = {}


def scratch_f32(device, n):
    """Grow-only f32 scratch per device for the fixed-order reductions (column sums, gradient norm, split-K
    slabs).  256 MiB to start with: 64 M floats hold 8 slabs of any weight gradient of the configs up to DiT-XL / ADM."""
    t = _scratch.get(device)
    if t is None or t.numel() < n:
        t = _scratch[device] = torch.empty(max(n, 1 << 26), device=device, dtype=torch.float32)
    return t


def colsum(dt, X, M, N, ldx, out, beta=0.0, device=None):
    need = L.lib().vaw_colsum_workspace_floats(M, N)
    ws = scratch_f32(device or torch.device("cuda", torch.cuda.current_device()), need)
    check(L.lib().vaw_colsum(dt, X, M, N, ldx, out, beta, ptr(ws), ws.numel(), stream_ptr()), "vaw_colsum")


# ---- DiT pieces (raw pointers; shapes are checked by the caller that owns the buffers) ---------------
def ln_modulate_fwd(dt, x, shift, scale, mod_ld, out, mean, rstd, B, T, D, eps=1e-6):
    check(L.lib().vaw_ln_modulate_fwd(dt, x, shift, scale, mod_ld, out, mean, rstd, B, T, D, eps, stream_ptr()),
          "vaw_ln_modulate_fwd")


def gate_resid_ln_modulate_fwd(dt, y, gate, gate_ld, x_in, x_out, shift, scale, mod_ld, out, mean, rstd, B, T, D, eps=1e-6):
    """x_out = y * gate + x_in and, unless out is 0, out / mean / rstd = ln_modulate_fwd of x_out, in one launch (bf16 rows)."""
    check(L.lib().vaw_gate_resid_ln_modulate_fwd(dt, y, gate, gate_ld, x_in, x_out, shift or None, scale or None, mod_ld, out or None,
                                                 mean or None, rstd or None, B, T, D, eps, stream_ptr()),
          "vaw_gate_resid_ln_modulate_fwd")


def ln_modulate_fwd_fp8(x, shift, scale, mod_ld, f8, mean, rstd, B, T, D, eps=1e-6, pool=2):
    """ln_modulate_fwd whose output goes straight into the Fp8 `f8` (row-major bytes + running max; delayed scaling state current)."""
    q = f8.epilogue_target(pool)
    check(L.lib().vaw_ln_modulate_fwd_fp8(x, shift, scale, mod_ld, q, f8.state.data_ptr(), f8.fmt, mean, rstd, B, T, D, eps, stream_ptr()),
          "vaw_ln_modulate_fwd_fp8")


def gate_bwd_fp8(dres, y, gate, mod_ld, f8, dgate, dmod_ld, B, T, D, dy_colpart=0, pool=2):
    """gate_bwd whose dy goes straight into the Fp8 `f8`."""
    ws = _row_ws(B, T, D)
    q = f8.epilogue_target(pool)
    check(L.lib().vaw_gate_bwd_fp8(dres, y, gate, mod_ld, q, f8.state.data_ptr(), f8.fmt, dgate, dmod_ld, dy_colpart or None, B, T, D,
                                   ws.data_ptr(), ws.numel(), stream_ptr()), "vaw_gate_bwd_fp8")


def row_plan(kind, dt, B, T, D, workspace_floats=0, ldx=0, base_addr=0):
    """The launch the row-kernel entry point `kind` (_lib.ROW_*) makes for these sizes (vaw_row_plan: host arithmetic, no GPU).
    Colsum: B = M rows, T = 1, D = N columns, ldx and the address of X."""
    p = L.RowLaunch()
    check(L.lib().vaw_row_plan(kind, dt, B, T, D, ldx, base_addr, workspace_floats, C.byref(p)), "vaw_row_plan")
    return p


def _row_ws(B, T, D):
    return scratch_f32(torch.device("cuda", torch.cuda.current_device()), L.lib().vaw_row_bwd_workspace_floats(B, T, D))


def ln_modulate_bwd(dt, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, B, T, D, dx_act=0):
    """dx_act: address of an act-dtype copy of dx the same launch leaves (0: none)."""
    ws = _row_ws(B, T, D)
    if dx_act:
        check(L.lib().vaw_ln_modulate_bwd_cast(dt, dout, x, mean, rstd, scale, mod_ld, dres_in or None, dx, dshift, dscale,
                                               dmod_ld, B, T, D, ws.data_ptr(), ws.numel(), dx_act, stream_ptr()), "vaw_ln_modulate_bwd_cast")
        return
    check(L.lib().vaw_ln_modulate_bwd(dt, dout, x, mean, rstd, scale, mod_ld, dres_in or None, dx, dshift, dscale,
                                      dmod_ld, B, T, D, ws.data_ptr(), ws.numel(), stream_ptr()), "vaw_ln_modulate_bwd")


def ln_modulate_bwd_gate(dt, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, y_next, gate_next, dy_next,
                         dgate_next, B, T, D, dy_colpart=0):
    """ln_modulate_bwd + the gate_bwd that consumes its dx, one pass (vaw_ln_modulate_bwd_gate: row_bwd_fuse8_kernel for bf16 rows up
    to 1280 wide -- per-sample sums in LDS slabs, operand rows requested ahead).  Wider rows run the pair instead (bitwise the same
    results): the fused kernel's LDS slabs no longer fit and the register-accumulator form held 16 waves per CU at 3.3 TB/s."""
    if D > 1280:
        ln_modulate_bwd(dt, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, B, T, D)
        gate_bwd(dt, dx, y_next, gate_next, mod_ld, dy_next, dgate_next, dmod_ld, B, T, D, dy_colpart)
        return
    ws = _row_ws(B, T, D)
    check(L.lib().vaw_ln_modulate_bwd_gate(dt, dout, x, mean, rstd, scale, mod_ld, dres_in or None, dx, dshift, dscale, dmod_ld,
                                           y_next, gate_next, dy_next, dgate_next, dy_colpart or None, B, T, D, ws.data_ptr(),
                                           ws.numel(), stream_ptr()), "vaw_ln_modulate_bwd_gate")


def ln_modulate_bwd_gate_fp8(dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, y_next, gate_next, f8,
                             dgate_next, B, T, D, dy_colpart=0, pool=2):
    """The fused pass with dy_next going straight into the Fp8 `f8` (as gate_bwd_fp8); wide rows: the pair, as above."""
    if D > 1280:
        ln_modulate_bwd(BF16, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, B, T, D)
        gate_bwd_fp8(dx, y_next, gate_next, mod_ld, f8, dgate_next, dmod_ld, B, T, D, dy_colpart, pool)
        return
    ws = _row_ws(B, T, D)
    q = f8.epilogue_target(pool)
    check(L.lib().vaw_ln_modulate_bwd_gate_fp8(dout, x, mean, rstd, scale, mod_ld, dres_in or None, dx, dshift, dscale, dmod_ld,
                                               y_next, gate_next, q, f8.state.data_ptr(), f8.fmt, dgate_next, dy_colpart or None,
                                               B, T, D, ws.data_ptr(), ws.numel(), stream_ptr()), "vaw_ln_modulate_bwd_gate_fp8")


class ColsumPartial:
    """Partial column sums [rows][N] f32 a dy-producing kernel leaves behind (rows: set by the kernel / known to the caller),
    folded later by a ReduceGroup."""

    def __init__(self, max_rows, N, device):
        self.buf = torch.empty(max_rows, N, device=device, dtype=torch.float32)
        self.N = int(N)
        self.rows = C.c_int64(0)


class ReduceGroup(TableGroup):
    """out_j = beta * out_j + column sums of partial_j for many (partial, out, R, N) jobs in ONE launch (vaw_reduce_rows_batched)."""

    def __init__(self, jobs, device):
        super().__init__(ReduceJob, [ReduceJob(*j) for j in jobs], L.lib().vaw_reduce_rows_batched_desc_bytes, device)

    def launch(self, beta):
        self._call("vaw_reduce_rows_batched", self.n, self.table, float(beta))


def gate_bwd(dt, dres, y, gate, mod_ld, dy, dgate, dmod_ld, B, T, D, dy_colpart=0):
    ws = _row_ws(B, T, D)
    check(L.lib().vaw_gate_bwd(dt, dres, y, gate, mod_ld, dy, dgate, dmod_ld, dy_colpart or None, B, T, D, ws.data_ptr(),
                               ws.numel(), stream_ptr()), "vaw_gate_bwd")


def reduce_rows(partial, R, N, out, beta):
    check(L.lib().vaw_reduce_rows(partial, R, N, out, beta, stream_ptr()), "vaw_reduce_rows")


def attn_desc_token_major(B, H, T, hd):
    """qkv rows [B*T, 3*H*hd] (timm Attention); output rows [B*T, H*hd]."""
    return AttnDesc(B, H, T, hd, T * 3 * H * hd, hd, 3 * H * hd, 1, T * H * hd, hd, H * hd, 1, hd ** -0.5)


def attn_desc_channel_major(B, H, T, ch):
    """qkv [B, 3*H*ch, T] (UNet QKVAttention, new order); output [B, H*ch, T]."""
    return AttnDesc(B, H, T, ch, 3 * H * ch * T, ch * T, 1, T, H * ch * T, ch * T, 1, T, ch ** -0.5)


def attn_desc_nhwc(B, H, T, ch, new_order):
    """qkv rows [B*T, 3*H*ch] (the UNet's attention on NHWC activations); channels [3][H][ch] (new order) or [H][3][ch]
    (legacy order); output rows [B*T, H*ch].  k and v start ko / vo elements after q: returns (desc, ko, vo)."""
    C_ = H * ch
    desc = AttnDesc(B, H, T, ch, T * 3 * C_, ch if new_order else 3 * ch, 3 * C_, 1, T * C_, ch, C_, 1, ch ** -0.5)
    return (desc, C_, 2 * C_) if new_order else (desc, ch, 2 * ch)


def attn_plan(direction, dt, desc, q, k, v, o_or_do, dq=0, dk=0, dv=0):
    """The launch the attention entry point `direction` (_lib.ATTN_FWD / ATTN_BWD / ATTN_BWD_COLSUM) makes for this descriptor
    and these addresses (vaw_attn_plan: host arithmetic, no GPU; o_or_do: o for the forward, d_o for the backward)."""
    p = L.AttnLaunch()
    check(L.lib().vaw_attn_plan(direction, dt, C.byref(desc), q, k, v, o_or_do, dq, dk, dv, C.byref(p)), "vaw_attn_plan")
    return p


def dit_ws_plan(dt, B, T, D, Dm, depth, heads, Kp, No, defer_wgrad=True, checkpoint=False):
    """Byte sizes of the DiT engine's activation workspace for these sizes (vaw_dit_ws_plan: host arithmetic, no GPU):
    what one block keeps resident, the record all blocks share under activation checkpointing, backward scratch, the total."""
    p = L.DitWsPlan()
    check(L.lib().vaw_dit_ws_plan(dt, B, T, D, Dm, depth, heads, Kp, No, int(defer_wgrad), int(checkpoint), C.byref(p)), "vaw_dit_ws_plan")
    return p


def attn_fwd(dt, desc, q, k, v, o, lse):
    check(L.lib().vaw_attn_fwd(dt, C.byref(desc), q, k, v, o, lse, stream_ptr()), "vaw_attn_fwd")


def attn_bwd(dt, desc, q, k, v, o, d_o, lse, delta, dq, dk, dv):
    check(L.lib().vaw_attn_bwd(dt, C.byref(desc), q, k, v, o, d_o, lse, delta, dq, dk, dv, stream_ptr()), "vaw_attn_bwd")


def attn_bwd_colsum(dt, desc, q, k, v, o, d_o, lse, delta, dq, dk, dv, partial):
    """attn_bwd that leaves the column sums of dq | dk | dv as partial rows in the ColsumPartial `partial` (the qkv bias
    gradient, folded later).  False -- nothing launched -- when the kernel path in use cannot (call attn_bwd + colsum then)."""
    partial.rows.value = partial.buf.shape[0]             # in: capacity; out: rows written
    rc = L.lib().vaw_attn_bwd_colsum(dt, C.byref(desc), q, k, v, o, d_o, lse, delta, dq, dk, dv, partial.buf.data_ptr(),
                                     C.byref(partial.rows), stream_ptr())
    if rc == -3:
        return False
    check(rc, "vaw_attn_bwd_colsum")
    return True


def timestep_embedding(t, dim, dtype=torch.float32, max_period=10000.0):
    """[cos | sin] embedding (tools/nn.py:103-121).  t: float tensor [B] on the GPU."""
    need_cuda(t)
    t = t.float().contiguous()
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=dtype)
    check(L.lib().vaw_timestep_embedding(dt_of(out), ptr(t), ptr(out), t.shape[0], dim, max_period, stream_ptr()),
          "vaw_timestep_embedding")
    return out


# ---- optimizer ---------------------------------------------------------------------------------
def sumsq(g, out, accumulate=False):
    ws = scratch_f32(g.device, L.lib().vaw_sumsq_workspace_floats())
    check(L.lib().vaw_sumsq(ptr(g), g.numel(), ptr(out), 1 if accumulate else 0, ptr(ws), stream_ptr()), "vaw_sumsq")


def adamw_ema_step(p, g, m, v, ema, shadow, lr, beta1, beta2, eps, wd, step, ema_decay, sumsq_t, clip, zero_grad, hyper=None, ok=None):
    """hyper: device f32[3] {lr, bc1, bc2} -- when given, the kernel reads the step-dependent scalars from it (graph replay).
    ok: device int32[1], the step guard's verdict -- when given, the guarded entry runs: the same pass where ok[0] != 0, nothing but
    the zero_grad store where it is 0."""
    if ok is not None:
        need_cuda(ok)
        zg = 1 if zero_grad else 0
        if hyper is not None:
            check(L.lib().vaw_adamw_ema_step_guarded_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(shadow), p.numel(), ptr(hyper),
                                                         beta1, beta2, eps, wd, ema_decay, ptr(sumsq_t), clip or 0.0, zg, ptr(ok),
                                                         stream_ptr()), "vaw_adamw_ema_step_guarded_dev")
            return
        check(L.lib().vaw_adamw_ema_step_guarded(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(shadow), p.numel(), lr, beta1, beta2,
                                                 eps, wd, 1.0 - beta1 ** step, 1.0 - beta2 ** step, ema_decay, ptr(sumsq_t), clip or 0.0,
                                                 zg, ptr(ok), stream_ptr()), "vaw_adamw_ema_step_guarded")
        return
    if hyper is not None:
        check(L.lib().vaw_adamw_ema_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(shadow), p.numel(), ptr(hyper), beta1,
                                             beta2, eps, wd, ema_decay, ptr(sumsq_t), clip or 0.0, 1 if zero_grad else 0,
                                             stream_ptr()), "vaw_adamw_ema_step_dev")
        return
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(L.lib().vaw_adamw_ema_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(shadow), p.numel(), lr, beta1, beta2,
                                     eps, wd, bc1, bc2, ema_decay, ptr(sumsq_t), clip or 0.0, 1 if zero_grad else 0,
                                     stream_ptr()), "vaw_adamw_ema_step")


def ema_update(ema, src, decay):
    check(L.lib().vaw_ema_update(ptr(ema), ptr(src), ema.numel(), decay, stream_ptr()), "vaw_ema_update")


# ---- post-hoc EMA (ema.py) ---------------------------------------------------------------------
def ema_profiles_coef(step, gamma, coef):
    """step i64 [1] += 1 (= t) and coef f64 [K] = c_t of the exponents gamma f64 [K], on the device: no host value in the launch."""
    need_cuda(step, gamma, coef)
    assert step.dtype == torch.int64 and step.numel() == 1 and gamma.dtype == coef.dtype == torch.float64
    assert gamma.is_contiguous() and coef.is_contiguous() and gamma.numel() == coef.numel()
    check(L.lib().vaw_ema_profiles_coef(ptr(step), ptr(gamma), ptr(coef), gamma.numel(), stream_ptr()), "vaw_ema_profiles_coef")


def ema_profiles_update(p, bufs, coef):
    """bufs[k] = c == 1 ? p : bufs[k] + (p - bufs[k]) * c with c = float32(coef[k]), for the len(bufs) averages in one pass over p.
    What the kernel cannot take (alignment, overlap, a count outside 1 .. EMA_MAX_PROFILES) it refuses: VawError, nothing launched."""
    need_cuda(p, coef, *bufs)
    _f32c(p, *bufs)
    assert coef.dtype == torch.float64 and coef.is_contiguous() and coef.numel() >= min(len(bufs), L.EMA_MAX_PROFILES)
    assert all(b.numel() == p.numel() for b in bufs)
    e = [ptr(b) for b in bufs[:L.EMA_MAX_PROFILES]] + [0] * (L.EMA_MAX_PROFILES - len(bufs))
    check(L.lib().vaw_ema_profiles_update(ptr(p), *e, len(bufs), p.numel(), ptr(coef), stream_ptr()), "vaw_ema_profiles_update")


def lincomb_accum_f64(acc, src, coef):
    """acc (f64) += coef * float64(src) (src f32), product and sum rounded separately; in place."""
    need_cuda(acc, src)
    _f32c(src)
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == src.numel()
    check(L.lib().vaw_lincomb_accum_f64(ptr(acc), ptr(src), float(coef), acc.numel(), stream_ptr()), "vaw_lincomb_accum_f64")


def f64_to_f32(acc, out):
    need_cuda(acc, out)
    _f32c(out)
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == out.numel()
    check(L.lib().vaw_f64_to_f32(ptr(acc), ptr(out), acc.numel(), stream_ptr()), "vaw_f64_to_f32")


def cast_bf16(src, dst):
    check(L.lib().vaw_cast_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()), "vaw_cast_bf16")


def cast_colsum_plan(M, N, ld_src, ld_dst, src_addr, dst_addr, colsum_addr):
    """The launch vaw_cast_colsum_bf16 makes for these operands, or None where it refuses them (host arithmetic, no GPU)."""
    p = L.CastColsumLaunch()
    rc = L.lib().vaw_cast_colsum_plan(M, N, ld_src, ld_dst, src_addr, dst_addr, colsum_addr, C.byref(p))
    return p if rc == 0 else None


def cast_colsum(src, ld_src, dst, ld_dst, M, N, colsum_out, beta=0.0):
    """dst (bf16) = src (f32) over [M][N] (raw addresses, row strides in elements) and colsum_out = beta * colsum_out + the column
    sums of dst, one launch; bitwise cast_bf16 followed by colsum.  Raises where vaw_cast_colsum_plan refuses."""
    check(L.lib().vaw_cast_colsum_bf16(src, ld_src, dst, ld_dst, M, N, colsum_out, beta, stream_ptr()), "vaw_cast_colsum_bf16")


def silu_bwd(x, dy, dx, dx_bf16=None):
    """dx = dy * silu'(x) (f32 tensors) and, when given, dx_bf16 = bf16(dx) from the same launch."""
    check(L.lib().vaw_silu_bwd_cast(ptr(x), ptr(dy), ptr(dx), ptr(dx_bf16), dx.numel(), stream_ptr()), "vaw_silu_bwd_cast")


def uncast_bf16(src, dst, scale=1.0):
    """dst (f32) = scale * src (bf16), on the current stream."""
    check(L.lib().vaw_uncast_bf16(ptr(src), ptr(dst), src.numel(), float(scale), stream_ptr()), "vaw_uncast_bf16")


# ---- UNet activation recomputation (unet.py: use_checkpoint) ------------------------------------------------
def gn_plan(gn_pass, dt, B, HW, C, G=32):
    """The launch the GroupNorm entry points make for the streaming pass `gn_pass` (_lib.GN_FWD_SUMS / GN_APPLY / GN_BWD_SUMS /
    GN_BWD_APPLY) at these sizes, under the vaw_debug_gn_flat switch as it stands (vaw_gn_plan: host arithmetic, no GPU)."""
    p = L.GnLaunch()
    check(L.lib().vaw_gn_plan(gn_pass, dt, B, HW, C, G, L.C.byref(p)), "vaw_gn_plan")
    return p


def groupnorm_apply(dt, x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, y, B, HW, C, G=32):
    """The apply pass of vaw_groupnorm_fwd on saved statistics (raw pointers; scale / shift 0 = no FiLM)."""
    check(L.lib().vaw_groupnorm_apply(dt, x, mean, rstd, gamma, beta, scale or None, shift or None, film_ld, 1 if silu else 0, y,
                                      B, HW, C, G, stream_ptr()), "vaw_groupnorm_apply")


def dropout_pack(dt, mask, M, C):
    """[M, C] act-dtype keep mask (keep ? 1/(1-p) : 0) -> int32 words, 1 bit per element."""
    bits = torch.empty(L.lib().vaw_dropout_bits_words(M * C), device=mask.device, dtype=torch.int32)
    check(L.lib().vaw_dropout_pack(dt, ptr(mask), ptr(bits), M, C, stream_ptr()), "vaw_dropout_pack")
    return bits


def dropout_bits(dt, x, bits, keep_scale, y, n, backward=False):
    """y = x * (bit ? keep_scale : 0): bitwise vaw_mul with the unpacked mask (raw pointers for x / y)."""
    fn = L.lib().vaw_dropout_bits_bwd if backward else L.lib().vaw_dropout_bits_fwd
    check(fn(dt, x, ptr(bits), keep_scale, y, n, stream_ptr()), "vaw_dropout_bits_bwd" if backward else "vaw_dropout_bits_fwd")


# ---- evaluation metrics from activations (evaluator.py; csrc/metrics.hip) -----------------------------------------
KSMALLEST_MAX = 16      # largest k1 of pairwise_ksmallest
WITHIN_MAX_RADII = 4    # most radii per point of pairwise_within


def _features(what, *ts):
    """f32, 2-D, contiguous CUDA tensors of one feature width."""
    need_cuda(*ts)
    for t in ts:
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{what}: features must be non-empty contiguous float32 [N, D] tensors, got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] != ts[0].shape[1]:
            raise ValueError(f"{what}: feature widths differ: {ts[0].shape[1]} and {t.shape[1]}")


def _per_row(what, name, t, rows, cols=None, dtype=torch.float32):
    need_cuda(t)
    want = (rows,) if cols is None else (rows, cols)
    if t.dtype != dtype or tuple(t.shape) != want or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {want}, got {t.dtype} {tuple(t.shape)}")


def row_sqnorms(x):
    """out[i] = sum_k x[i][k]^2 (f32, fixed order)."""
    _features("row_sqnorms", x)
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    check(L.lib().vaw_row_sqnorms(ptr(x), x.shape[0], x.shape[1], ptr(out), stream_ptr()), "vaw_row_sqnorms")
    return out


def pairwise_ksmallest(u, v, k1, norm_u=None, norm_v=None):
    """[nu, k1]: per row of u the k1 smallest squared distances max((|u|^2 - 2 u.v) + |v|^2, 0) to the rows of v, ascending."""
    _features("pairwise_ksmallest", u, v)
    nu, nv = u.shape[0], v.shape[0]
    if not 1 <= k1 <= min(KSMALLEST_MAX, nv):
        raise ValueError(f"pairwise_ksmallest: k1 = {k1} outside 1 .. min({KSMALLEST_MAX}, nv = {nv})")
    norm_u = row_sqnorms(u) if norm_u is None else norm_u
    norm_v = (norm_u if v is u else row_sqnorms(v)) if norm_v is None else norm_v
    _per_row("pairwise_ksmallest", "norm_u", norm_u, nu)
    _per_row("pairwise_ksmallest", "norm_v", norm_v, nv)
    nbytes = L.lib().vaw_pairwise_workspace_bytes(nu, nv, k1)
    ws = torch.empty(nbytes // 4, device=u.device, dtype=torch.float32)
    out = torch.empty(nu, k1, device=u.device, dtype=torch.float32)
    check(L.lib().vaw_pairwise_ksmallest(ptr(u), nu, ptr(v), nv, u.shape[1], ptr(norm_u), ptr(norm_v), k1, ptr(out), ptr(ws), nbytes,
                                         stream_ptr()), "vaw_pairwise_ksmallest")
    return out


def ksmallest_merge(parts):
    """parts [P, n, k1] (ascending or not, +inf = empty) -> [n, k1]: the k1 smallest of each row's P * k1 values, ascending."""
    need_cuda(parts)
    if parts.dtype != torch.float32 or parts.dim() != 3 or not parts.is_contiguous() or not 1 <= parts.shape[2] <= KSMALLEST_MAX:
        raise ValueError(f"ksmallest_merge: parts must be contiguous float32 [P, n, k1 <= {KSMALLEST_MAX}], got {parts.dtype} {tuple(parts.shape)}")
    P, n, k1 = parts.shape
    out = torch.empty(n, k1, device=parts.device, dtype=torch.float32)
    check(L.lib().vaw_ksmallest_merge(ptr(parts), n, P, k1, n * k1, k1, ptr(out), stream_ptr()), "vaw_ksmallest_merge")
    return out


def pairwise_within(u, v, norm_u, norm_v, radii_u, radii_v, u_in, v_in):
    """u_in[i][c] |= any_j d(i, j) <= radii_v[j][c] and v_in[j][c] |= any_i d(i, j) <= radii_u[i][c] (uint8 flags, zeroed by the
    caller before the first call)."""
    _features("pairwise_within", u, v)
    nu, nv = u.shape[0], v.shape[0]
    for name, r in (("radii_u", radii_u), ("radii_v", radii_v)):
        if r.dim() != 2 or not 1 <= r.shape[1] <= WITHIN_MAX_RADII:
            raise ValueError(f"pairwise_within: {name} must be [N, 1 .. {WITHIN_MAX_RADII}], got {tuple(r.shape)}")
    Ku, Kv = radii_u.shape[1], radii_v.shape[1]
    _per_row("pairwise_within", "norm_u", norm_u, nu)
    _per_row("pairwise_within", "norm_v", norm_v, nv)
    _per_row("pairwise_within", "radii_u", radii_u, nu, Ku)
    _per_row("pairwise_within", "radii_v", radii_v, nv, Kv)
    _per_row("pairwise_within", "u_in", u_in, nu, Kv, torch.uint8)
    _per_row("pairwise_within", "v_in", v_in, nv, Ku, torch.uint8)
    check(L.lib().vaw_pairwise_within(ptr(u), nu, ptr(v), nv, u.shape[1], ptr(norm_u), ptr(norm_v), ptr(radii_u), Ku, ptr(radii_v), Kv,
                                      ptr(u_in), ptr(v_in), stream_ptr()), "vaw_pairwise_within")


POLYSUM_MAX_DEGREE = 8  # largest degree of pairwise_polysum


def _index_table(what, name, idx, rows, device):
    """An index table as contiguous int32 [batches, n] on the device.  The values are checked on the host before the upload: the
    kernel reads the rows they name without a check of its own."""
    if isinstance(idx, torch.Tensor):
        if idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError(f"{what}: {name} must be a non-empty int32 / int64 [batches, n] table, got {idx.dtype} {tuple(idx.shape)}")
        lo, hi = int(idx.min()), int(idx.max())
    else:
        idx = np.asarray(idx)
        if idx.dtype.kind not in "iu" or idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError(f"{what}: {name} must be a non-empty integer [batches, n] table, got {idx.dtype} {idx.shape}")
        lo, hi = int(idx.min()), int(idx.max())
        idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32 if hi < 2 ** 31 else np.int64))
    if lo < 0 or hi >= rows:
        raise ValueError(f"{what}: {name} holds values {lo} .. {hi} outside the rows 0 .. {rows - 1}")
    return idx.to(device=device, dtype=torch.int32).contiguous()


def pairwise_polysum(u, v, gamma, coef0, degree, u_idx=None, v_idx=None, skip_diagonal=False):
    """float64 [batches, nu]: out[b][i] = sum_j (gamma * u[u_idx[b][i]] . v[v_idx[b][j]] + coef0)^degree in a fixed order, the dot
    product the f32 MFMA chain of the distances.  u_idx [batches, nu] / v_idx [batches, nv] pick rows of u / v (None: all rows, in
    order, for every batch).  skip_diagonal leaves out the pairs whose two indices are equal."""
    _features("pairwise_polysum", u, v)
    if isinstance(degree, bool) or int(degree) != degree or not 1 <= degree <= POLYSUM_MAX_DEGREE:
        raise ValueError(f"pairwise_polysum: degree must be an integer in 1 .. {POLYSUM_MAX_DEGREE}, got {degree}")
    gamma, coef0 = float(gamma), float(coef0)
    if not (math.isfinite(gamma) and math.isfinite(coef0)):
        raise ValueError(f"pairwise_polysum: gamma = {gamma} and coef0 = {coef0} must be finite")
    if u_idx is not None:
        u_idx = _index_table("pairwise_polysum", "u_idx", u_idx, u.shape[0], u.device)
    if v_idx is not None:
        v_idx = _index_table("pairwise_polysum", "v_idx", v_idx, v.shape[0], u.device)
    tables = [t for t in (u_idx, v_idx) if t is not None]
    batches = tables[0].shape[0] if tables else 1
    if any(t.shape[0] != batches for t in tables):
        raise ValueError(f"pairwise_polysum: u_idx and v_idx hold {u_idx.shape[0]} and {v_idx.shape[0]} batches")
    nu = u.shape[0] if u_idx is None else u_idx.shape[1]
    nv = v.shape[0] if v_idx is None else v_idx.shape[1]
    nbytes = L.lib().vaw_pairwise_polysum_workspace_bytes(nu, nv, batches)
    ws = torch.empty(nbytes // 8, device=u.device, dtype=torch.float64)
    out = torch.empty(batches, nu, device=u.device, dtype=torch.float64)
    check(L.lib().vaw_pairwise_polysum(ptr(u), nu, ptr(v), nv, u.shape[1], ptr(u_idx), ptr(v_idx), batches, gamma, coef0, int(degree),
                                       int(bool(skip_diagonal)), ptr(out), ptr(ws), nbytes, stream_ptr()), "vaw_pairwise_polysum")
    return out


def pairwise_count_within(u, v, norm_u, norm_v, radii_v, u_count, v_in):
    """u_count[i][c] += #{ j : d(i, j) < radii_v[j][c] } (int32) and v_in[j][c] |= any_i d(i, j) < radii_v[j][c] (uint8), strictly
    below where pairwise_within takes <=; both zeroed by the caller before the first call."""
    _features("pairwise_count_within", u, v)
    nu, nv = u.shape[0], v.shape[0]
    need_cuda(radii_v)
    if radii_v.dim() != 2 or not 1 <= radii_v.shape[1] <= WITHIN_MAX_RADII:
        raise ValueError(f"pairwise_count_within: radii_v must be [N, 1 .. {WITHIN_MAX_RADII}], got {tuple(radii_v.shape)}")
    Kv = radii_v.shape[1]
    _per_row("pairwise_count_within", "norm_u", norm_u, nu)
    _per_row("pairwise_count_within", "norm_v", norm_v, nv)
    _per_row("pairwise_count_within", "radii_v", radii_v, nv, Kv)
    _per_row("pairwise_count_within", "u_count", u_count, nu, Kv, torch.int32)
    _per_row("pairwise_count_within", "v_in", v_in, nv, Kv, torch.uint8)
    nbytes = L.lib().vaw_pairwise_count_workspace_bytes(nu, nv, Kv)
    ws = torch.empty(nbytes // 4, device=u.device, dtype=torch.int32)
    check(L.lib().vaw_pairwise_count_within(ptr(u), nu, ptr(v), nv, u.shape[1], ptr(norm_u), ptr(norm_v), ptr(radii_v), Kv, ptr(u_count),
                                            ptr(v_in), ptr(ws), nbytes, stream_ptr()), "vaw_pairwise_count_within")


def col_mean_f64(x):
    """f64 [D]: the column means of f32 x [n, D]."""
    _features("col_mean_f64", x)
    mu = torch.empty(x.shape[1], device=x.device, dtype=torch.float64)
    check(L.lib().vaw_col_mean_f64(ptr(x), x.shape[0], x.shape[1], ptr(mu), stream_ptr()), "vaw_col_mean_f64")
    return mu


def cov_f64(x, mu):
    """f64 [D, D]: (x - mu)^T (x - mu) / (n - 1), centred and two-pass, symmetric bit for bit."""
    _features("cov_f64", x)
    _per_row("cov_f64", "mu", mu, x.shape[1], dtype=torch.float64)
    sigma = torch.empty(x.shape[1], x.shape[1], device=x.device, dtype=torch.float64)
    check(L.lib().vaw_cov_f64(ptr(x), x.shape[0], x.shape[1], ptr(mu), ptr(sigma), stream_ptr()), "vaw_cov_f64")
    return sigma


def _rows_f32(what, name, t):
    """f32 [n, C] on the GPU with unit column stride, rows at least C apart (a row-strided view of a wider buffer is fine)."""
    need_cuda(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: {name} must be a non-empty float32 [n, C] tensor with unit column stride, got {t.dtype} {tuple(t.shape)} "
                         f"strides {tuple(t.stride())}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def head_logits(x, wt, out=None):
    """f32 [n, C]: out[i][c] = sum_k x[i][k] wt[c][k] for x [n, D] and the class-major weight wt [C, D], every element one ordered
    f32 MFMA chain.  `out` may be a row-strided view; nothing outside its n x C elements is written."""
    _features("head_logits", x, wt)
    n, C = x.shape[0], wt.shape[0]
    if out is None:
        out = torch.empty(n, C, device=x.device, dtype=torch.float32)
    ld = _rows_f32("head_logits", "out", out)
    if tuple(out.shape) != (n, C):
        raise ValueError(f"head_logits: out must be of shape {(n, C)}, got {tuple(out.shape)}")
    check(L.lib().vaw_head_logits(ptr(x), n, x.shape[1], ptr(wt), C, ptr(out), ld, stream_ptr()), "vaw_head_logits")
    return out


def is_rows(rows, probs=False, lse=None, h=None):
    """(lse, h), float64 [n]: of every row of logits its log-sum-exp and sum_c p_c (l_c - lse) with p = softmax; with probs=True the
    rows are probabilities, h = sum_c p_c log p_c (0 log 0 = 0) and lse is 0."""
    ld = _rows_f32("is_rows", "rows", rows)
    n, C = rows.shape
    lse = torch.empty(n, device=rows.device, dtype=torch.float64) if lse is None else lse
    h = torch.empty(n, device=rows.device, dtype=torch.float64) if h is None else h
    _per_row("is_rows", "lse", lse, n, dtype=torch.float64)
    _per_row("is_rows", "h", h, n, dtype=torch.float64)
    check(L.lib().vaw_is_rows(ptr(rows), n, C, ld, int(bool(probs)), ptr(lse), ptr(h), stream_ptr()), "vaw_is_rows")
    return lse, h


def is_colsums(rows, lse, row0, split_size, colsum, probs=False):
    """colsum[s][c] += the probabilities of the rows (global rows row0 .. row0 + n) that lie in split s, each (s, c) one float64
    chain in ascending row order which a later call continues; calls come in ascending row0.  colsum: float64 [splits, C]."""
    ld = _rows_f32("is_colsums", "rows", rows)
    n, C = rows.shape
    row0, split_size = int(row0), int(split_size)
    if row0 < 0 or split_size < 1:
        raise ValueError(f"is_colsums: row0 = {row0}, split_size = {split_size} out of range")
    if not probs:
        _per_row("is_colsums", "lse", lse, n, dtype=torch.float64)
    need_cuda(colsum)
    if colsum.dtype != torch.float64 or colsum.dim() != 2 or not colsum.is_contiguous() or colsum.shape[1] != C \
            or colsum.shape[0] * split_size < row0 + n:
        raise ValueError(f"is_colsums: colsum must be a contiguous float64 [splits >= {-(-(row0 + n) // split_size)}, {C}] tensor, got "
                         f"{colsum.dtype} {tuple(colsum.shape)}")
    check(L.lib().vaw_is_colsums(ptr(rows), None if probs else ptr(lse), n, C, ld, int(bool(probs)), row0, split_size, ptr(colsum), stream_ptr()),
          "vaw_is_colsums")


def is_finish(h, colsum, split_size):
    """float64 [splits]: exp(mean_i h_i - sum_c m_c log m_c) per split of split_size rows (the last one ragged), m = colsum / rows."""
    need_cuda(h, colsum)
    split_size = int(split_size)
    if h.dtype != torch.float64 or h.dim() != 1 or not h.is_contiguous() or h.shape[0] < 1 or split_size < 1:
        raise ValueError(f"is_finish: h must be a non-empty contiguous float64 [N] tensor and split_size >= 1, got {h.dtype} {tuple(h.shape)}, {split_size}")
    N = h.shape[0]
    S = -(-N // split_size)
    if colsum.dtype != torch.float64 or colsum.dim() != 2 or not colsum.is_contiguous() or colsum.shape[0] != S or colsum.shape[1] < 1:
        raise ValueError(f"is_finish: colsum must be a contiguous float64 [{S}, C] tensor, got {colsum.dtype} {tuple(colsum.shape)}")
    scores = torch.empty(S, device=h.device, dtype=torch.float64)
    check(L.lib().vaw_is_finish(ptr(h), ptr(colsum), N, colsum.shape[1], split_size, ptr(scores), stream_ptr()), "vaw_is_finish")
    return scores

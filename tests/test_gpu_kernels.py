"""Parity of each HIP kernel (through the C ABI, libvaw_hip.so) with the CPU oracle / a float64 torch
statement of the same op, on seeded inputs.  Run on the MI355X box: pytest -m gpu."""
import math

import numpy as np
import os

import pytest
import torch

from conftest import base_args, fake_model, load_json, load_pt

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, lib, ptr, stream_ptr

from oracle import diffusion as od

DEV = "cuda"


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------
# diffusion objective
# ------------------------------------------------------------------------------------------------
def _pair(sched="cosine", mt="EPSILON", wt="lambda"):
    kw = dict(args=base_args(weight_type=wt), model_var_type=None, loss_type=None, rescale_timesteps=True)
    o = od.GaussianDiffusion(betas=od.get_named_beta_schedule(sched, 1000), model_mean_type=od.ModelMeanType[mt],
                             **{**kw, "model_var_type": od.ModelVarType.FIXED_LARGE, "loss_type": od.LossType.MSE})
    p = vaw_amd.GaussianDiffusion(betas=vaw_amd.get_named_beta_schedule(sched, 1000),
                                  model_mean_type=vaw_amd.ModelMeanType[mt],
                                  **{**kw, "model_var_type": vaw_amd.ModelVarType.FIXED_LARGE,
                                     "loss_type": vaw_amd.LossType.MSE})
    return o, p


def test_qsample_bit_exact_vs_oracle_and_golden():
    g = load_pt("objective.pt")
    x0, noise, t = g["x0"], g["noise"], g["t"]
    for sched in ("cosine", "linear"):
        o, p = _pair(sched)
        got = p.q_sample(x0.to(DEV), t.to(DEV), noise.to(DEV)).cpu()
        assert torch.equal(got, g[f"{sched}/EPSILON/x_t"]) and torch.equal(got, o.q_sample(x0, t, noise))
    # ragged per-sample size (not a multiple of 4) and a big batch
    o, p = _pair()
    x = _rand(37, 3, 5, 7, seed=1); n = _rand(37, 3, 5, 7, seed=2)
    tt = torch.randint(0, 1000, (37,), generator=torch.Generator().manual_seed(3))
    assert torch.equal(p.q_sample(x.to(DEV), tt.to(DEV), n.to(DEV)).cpu(), o.q_sample(x, tt, n))
    bad = p.q_sample(x.to(DEV), torch.full((37,), 1000).to(DEV), n.to(DEV))
    assert torch.isnan(bad).all()          # out-of-range timestep poisons the row instead of reading out of bounds


@pytest.mark.parametrize("mt", ["EPSILON", "START_X", "VELOCITY"])
@pytest.mark.parametrize("wt", ["lambda", "constant", "min_snr_5"])
def test_training_losses_vs_golden(mt, wt):
    g = load_pt("objective.pt")
    x0, noise, t, y = (g[k].to(DEV) for k in ("x0", "noise", "t", "y"))
    for sched in ("cosine", "linear"):
        _, p = _pair(sched, mt, wt)
        terms = p.training_losses(fake_model, x0, None, t=t, model_kwargs={"y": y}, noise=noise)
        torch.testing.assert_close(terms["mse"].cpu(), g[f"{sched}/{mt}/{wt}/mse"], rtol=2e-6, atol=1e-9)
        assert terms["loss"] is terms["mse"]
        if wt == "lambda":
            torch.testing.assert_close(p.compute_target(x0, noise, t).cpu(), g[f"{sched}/{mt}/target"], rtol=1e-6, atol=1e-7)


VB_CASES = [(sched, mt, vt, lt) for sched in ("cosine", "linear") for mt in ("EPSILON", "START_X")
            for vt in ("LEARNED_RANGE", "LEARNED", "FIXED_LARGE", "FIXED_SMALL") for lt in ("MSE", "RESCALED_MSE", "KL", "RESCALED_KL")
            if vt.startswith("LEARNED") or lt in ("KL", "RESCALED_KL")]


def test_variational_bound_objectives_vs_reference_golden():
    """Learned-variance vb term + pure KL losses on the fused vaw_vb_fwd/bwd kernels vs the values and output gradients
    the unmodified reference produced (tests/golden/vb_objective.pt): t = 0 takes the decoder-NLL branch, x0 holds
    values in the open-ended bins.  Tolerance 1e-4 relative (north star), far looser than the observed error."""
    g = load_pt("vb_objective.pt")
    x0, noise, t = (g[k].to(DEV) for k in ("x0", "noise", "t"))
    for sched, mt, vt, lt in VB_CASES:
        learned = vt.startswith("LEARNED")
        d = vaw_amd.GaussianDiffusion(args=base_args(weight_type="lambda", learn_sigma=learned),
                                      betas=vaw_amd.get_named_beta_schedule(sched, 1000),
                                      model_mean_type=vaw_amd.ModelMeanType[mt], model_var_type=vaw_amd.ModelVarType[vt],
                                      loss_type=vaw_amd.LossType[lt], rescale_timesteps=True)
        P = (g["P"] if learned else g["P"][:, :3]).clone().to(DEV).requires_grad_(True)
        terms = d.training_losses(lambda x, ts, **kw: P, x0, None, t=t, noise=noise)
        terms["loss"].sum().backward()
        key = f"{sched}/{mt}/{vt}/{lt}"
        # near-zero KLs (t = 999: five O(1) terms cancelling to 1e-6) carry f32 rounding of the O(1) terms: absolute floor
        floor = 2e-6 * (1000.0 if lt == "RESCALED_KL" else 1.0)
        for k, v in terms.items():
            torch.testing.assert_close(v.detach().cpu(), g[f"{key}/{k}"], rtol=1e-4, atol=floor, msg=f"{key}/{k}")
        ref = g[f"{key}/dP"]
        torch.testing.assert_close(P.grad.cpu(), ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()), msg=key + "/dP")


def test_sampling_side_vs_reference_golden():
    """SpacedDiffusion + p_sample / ddim_sample loops on the fused vaw_sample_step kernel vs trajectories the unmodified
    reference produced on CPU (tests/golden/sampling.pt); the stand-in denoiser runs in torch on the GPU, the per-step
    noise comes from the CPU RNG stream (args.cpu_rng) exactly as the reference drew it.  10..50 chained steps."""
    from conftest import SAMPLING_CASES, sampling_model, sampling_model_2c
    g = load_pt("sampling.pt")
    for k, v in g["space"].items():
        assert sorted(vaw_amd.space_timesteps(1000, k)) == v, k
    assert sorted(vaw_amd.space_timesteps(300, [10, 15, 20])) == g["space_300_10_15_20"]
    with pytest.raises(ValueError):
        vaw_amd.space_timesteps(1000, "ddim999")
    shape, y = (3, 3, 8, 8), torch.tensor([1, 5, 9], device=DEV)
    for name, sched, mt, vt, respacing, kind, eta, clip in SAMPLING_CASES:
        learned = vt.startswith("LEARNED")
        d = vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(1000, respacing),
                                    args=base_args(learn_sigma=learned, cpu_rng=True),
                                    betas=vaw_amd.get_named_beta_schedule(sched, 1000), model_mean_type=vaw_amd.ModelMeanType[mt],
                                    model_var_type=vaw_amd.ModelVarType[vt], loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        exp = g["loops"][name]
        assert d.timestep_map == exp["timestep_map"].tolist()
        torch.manual_seed(123)
        model = sampling_model_2c if learned else sampling_model
        kw = dict(clip_denoised=clip, model_kwargs={"y": y}, device=DEV)
        loop = d.ddim_sample_loop_progressive(model, shape, eta=eta, **kw) if kind == "ddim" else d.p_sample_loop_progressive(model, shape, **kw)
        traj = [o["sample"].cpu() for o in loop]
        assert len(traj) == exp["n"]
        for k, v in (("first", traj[0]), ("mid", traj[len(traj) // 2]), ("final", traj[-1])):
            torch.testing.assert_close(v, exp[k], rtol=1e-4, atol=1e-4, msg=f"{name}/{k}")
    # p_mean_variance keys and shapes; unsupported hooks fail loudly
    d = vaw_amd.GaussianDiffusion(args=base_args(), betas=vaw_amd.get_named_beta_schedule("linear", 100),
                                  model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_SMALL,
                                  loss_type=vaw_amd.LossType.MSE)
    x = torch.randn(2, 3, 4, 4, device=DEV)
    out = d.p_mean_variance(sampling_model, x, torch.tensor([0, 99], device=DEV))
    assert set(out) == {"mean", "variance", "log_variance", "pred_xstart"} and out["mean"].shape == x.shape
    assert float(out["pred_xstart"].abs().max()) <= 1.0
    with pytest.raises(NotImplementedError):
        d.p_sample(sampling_model, x, torch.tensor([0, 99], device=DEV), cond_fn=lambda *a: None)
    # IntervalCFG on the GPU
    xg, yy = g["cfg_x"].to(DEV), g["cfg_y"].to(DEV)
    for nm, scale, interval, tval in [("plain", 1.0, (-1.0, -1.0), 500.0), ("always", 2.5, (-1.0, -1.0), 500.0),
                                      ("inside", 1.8, (100.0, 600.0), 300.0), ("outside", 1.8, (100.0, 600.0), 800.0)]:
        m = vaw_amd.IntervalCFG(sampling_model, 10, scale, interval, True)
        torch.testing.assert_close(m(xg, torch.full((4,), tval, device=DEV), y=yy).cpu(), g["cfg"][nm], rtol=1e-5, atol=1e-6)


def test_wmse_backward_matches_autograd():
    o, p = _pair("cosine", "VELOCITY", "min_snr_5")
    x0, noise = _rand(6, 3, 9, 5, seed=4), _rand(6, 3, 9, 5, seed=5)
    t = torch.tensor([0, 5, 250, 500, 998, 999])
    out = _rand(6, 3, 9, 5, seed=6).requires_grad_(True)
    ref = o.training_losses(lambda x, tt, **k: out, x0, None, t=t, noise=noise)["mse"]
    gm = _rand(6, seed=7)
    (ref * gm).sum().backward()
    outd = out.detach().to(DEV).requires_grad_(True)
    got = p.training_losses(lambda x, tt, **k: outd, x0.to(DEV), None, t=t.to(DEV), noise=noise.to(DEV))["mse"]
    (got * gm.to(DEV)).sum().backward()
    torch.testing.assert_close(got.detach().cpu(), ref.detach(), rtol=2e-6, atol=1e-9)
    torch.testing.assert_close(outd.grad.cpu(), out.grad, rtol=2e-6, atol=1e-7)   # atol: cancellation in (out - target)


def test_flow_matching_vs_golden():
    g = load_pt("objective.pt")
    x0, noise, y, tf = (g[k].to(DEV) for k in ("x0", "noise", "y", "flow/t"))
    for path in ("linear", "cosine", "linear_logsnr"):
        for mt in ("VECTOR", "EPSILON", "VELOCITY", "START_X"):
            fm = vaw_amd.FlowMatching(args=base_args(path_type=path), model_mean_type=vaw_amd.ModelMeanType[mt])
            terms = fm.training_losses(fake_model, x0, None, t=tf, model_kwargs={"y": y}, noise=noise)
            torch.testing.assert_close(terms["mse"].cpu(), g[f"flow/{path}/{mt}/mse"], rtol=5e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------
# GEMM: three operand layouts x {f32 generic, bf16 generic, bf16 MFMA fast} x epilogues
# ------------------------------------------------------------------------------------------------
def _gemm_ref(A, B, a_k, b_k):
    Am = A.double() if a_k else A.double().t()
    Bm = B.double().t() if b_k else B.double()
    return Am @ Bm


def _mk(M, N, K, a_k, b_k, dtype, seed, ints=False):
    g = torch.Generator().manual_seed(seed)
    def r(*s):
        if ints:
            return torch.randint(-3, 4, s, generator=g).float()
        return torch.randn(*s, generator=g)
    A = r(M, K) if a_k else r(K, M)
    B = r(N, K) if b_k else r(K, N)
    return A.to(dtype), B.to(dtype)


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("mode", ["f32", "bf16_generic", "bf16_fast", "bf16_big", "bf16_p8_256", "bf16_p8_192", "bf16_sm64", "bf16_sm128", "bf16_sm128x128"])
def test_gemm_layouts_exact_integers(a_k, b_k, mode):
    """Small-integer operands are exact in bf16 and f32: any fragment-layout or swizzle error shows as a
    wrong integer, with asymmetric data on both sides (a symmetric operand would hide a transpose)."""
    dtype = torch.float32 if mode == "f32" else torch.bfloat16
    # the MFMA path predicates edge tiles: any M (multiple of 8 when A is mn-major), N % 8 == 0, K % 64 == 0
    shapes = ([(256, 384, 192), (200, 72, 128), (136, 200, 64), (192, 1728, 256), (64, 64, 64)] if mode == "bf16_fast"
              else [(256, 384, 192), (200, 72, 128), (136, 200, 64), (520, 264, 256), (304, 776, 320), (1024, 512, 2048)]
              if mode == "bf16_big" else
              # persistent kernel: edge tiles in M and N, one K tile only, more items than CUs (two items per workgroup)
              [(256, 384, 192), (200, 72, 128), (136, 200, 64), (520, 264, 256), (304, 776, 320), (1024, 512, 2048),
               (8192, 3072, 128), (4104, 2504, 192)]
              if mode.startswith("bf16_p8") else [(256, 384, 192), (70, 45, 23), (129, 1, 17), (5, 200, 64)])
    if mode.startswith("bf16_"):
        dtype = torch.bfloat16
    if mode.startswith("bf16_sm"):
        # the small-M kernel (64-row tiles, deep LDS-DMA ring; A k-major only): edge tiles in M and N, K of one tile (ring never
        # fills), of exactly / fewer / more tiles than the ring is deep, many tiles per XCD run
        if not a_k:
            pytest.skip("gemm_sm takes A k-major (forward / input-gradient layouts)")
        shapes = [(256, 384, 192), (200, 72, 128), (136, 200, 64), (520, 264, 256), (304, 776, 320), (64, 64, 64), (2048, 768, 768),
                  (1000, 3072, 128), (4096, 128, 3072)]
    lib().vaw_debug_force_generic_gemm(1 if mode == "bf16_generic" else 0)
    lib().vaw_debug_gemm_tile({"bf16_fast": 0, "bf16_big": 1, "bf16_p8_256": 2, "bf16_p8_192": 3, "bf16_sm64": 6, "bf16_sm128": 7, "bf16_sm128x128": 8}.get(mode, -1))
    try:
        for (M, N, K) in shapes:
            A, B = _mk(M, N, K, a_k, b_k, dtype, seed=M + N + K, ints=True)
            Ad, Bd = A.to(DEV), B.to(DEV)
            if mode in ("bf16_fast", "bf16_big", "bf16_p8_256", "bf16_p8_192", "bf16_sm64", "bf16_sm128", "bf16_sm128x128"):
                assert lib().vaw_gemm_uses_bf16_mfma(BF16, M, N, K, ptr(Ad), Ad.shape[1], ptr(Bd), Bd.shape[1]) == 1
            got = ops.gemm_t(Ad, Bd, a_kmajor=a_k, b_kmajor=b_k, out_dtype=torch.float32).cpu()
            ref = _gemm_ref(A, B, a_k, b_k)
            assert torch.equal(got.double(), ref), (mode, a_k, b_k, M, N, K, (got.double() - ref).abs().max())
            # bf16 output + fused column sums on edge tiles
            cs = torch.zeros(N, device=DEV)
            got2 = ops.gemm_t(Ad, Bd, a_kmajor=a_k, b_kmajor=b_k, colsum_out=cs).cpu()
            assert torch.equal(got2.double(), ref.to(dtype).double())
            torch.testing.assert_close(cs.cpu().double(), ref.to(dtype).double().sum(0), rtol=1e-6, atol=1e-3)
    finally:
        lib().vaw_debug_force_generic_gemm(0)
        lib().vaw_debug_gemm_tile(-1)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, False)])
def test_gemm_bf16_fast_random_and_large_k(a_k, b_k, tile):
    lib().vaw_debug_gemm_tile(tile)
    try:
        for (M, N, K) in [(128, 128, 64), (512, 256, 768), (256, 128, 3072), (768, 768, 16384)]:
            A, B = _mk(M, N, K, a_k, b_k, torch.bfloat16, seed=K)
            got = ops.gemm_t(A.to(DEV), B.to(DEV), a_kmajor=a_k, b_kmajor=b_k, out_dtype=torch.float32).cpu()
            ref = _gemm_ref(A, B, a_k, b_k)
            torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-3 * math.sqrt(K) * 0.05)
    finally:
        lib().vaw_debug_gemm_tile(-1)


@pytest.mark.parametrize("dtype,tile", [(torch.float32, -1), (torch.bfloat16, 0), (torch.bfloat16, 1), (torch.bfloat16, 2),
                                        (torch.bfloat16, 3), (torch.bfloat16, 5), (torch.bfloat16, 8)])
def test_gemm_epilogues(dtype, tile):
    lib().vaw_debug_gemm_tile(tile)
    try:
        _gemm_epilogues(dtype)
    finally:
        lib().vaw_debug_gemm_tile(-1)


def _gemm_epilogues(dtype):
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    Bt, T, N, K = 4, 32, 256, 128
    M = Bt * T
    A, W = _mk(M, N, K, True, True, dtype, seed=11)
    bias, gate = _rand(N, seed=12), _rand(Bt, 3 * N, seed=13)
    resid, rowadd = _rand(M, N, seed=14), _rand(T, N, seed=15)
    acc = A.double() @ W.double().t() + bias.double()
    d = lambda t: None if t is None else t.to(DEV)
    # bias only, act-dtype output
    got = ops.gemm_t(d(A), d(W), bias=d(bias))
    torch.testing.assert_close(got.cpu().double(), acc, **tol)
    # GELU(tanh) forward with saved pre-activation
    got, pre = ops.gemm_t(d(A), d(W), bias=d(bias), act=1, want_aux=True)
    torch.testing.assert_close(pre.cpu().double(), acc, **tol)
    torch.testing.assert_close(got.cpu().double(), torch.nn.functional.gelu(pre.cpu().double(), approximate="tanh"), **tol)
    # gated residual with saved branch output, f32 residual stream out
    gsl = gate[:, N:2 * N].contiguous()
    out = torch.empty(M, N, device=DEV)
    aux = torch.empty(M, N, device=DEV, dtype=dtype)
    gd, rd, Ad, Wd, bd = d(gate), d(resid), d(A), d(W), d(bias)     # keep the device copies alive across the launch
    ops.gemm(ops.dt_of(A), 1, 1, M, N, K, ptr(Ad), K, ptr(Wd), K, ptr(out), N, bias=ptr(bd), aux_out=ptr(aux),
             gate=ptr(gd) + 4 * N, gate_ld=3 * N, resid=ptr(rd), rows_per_batch=T, out_f32=True)
    y = aux.cpu().double()
    torch.testing.assert_close(y, acc, **tol)
    ref = resid.double() + gsl.double().repeat_interleave(T, 0) * y
    torch.testing.assert_close(out.cpu().double(), ref, **tol)
    # pos-embed row add
    got = ops.gemm_t(d(A), d(W), bias=d(bias), rowadd=d(rowadd), rows_per_batch=T, out_dtype=torch.float32)
    torch.testing.assert_close(got.cpu().double(), acc + rowadd.double().repeat(Bt, 1), **tol)
    # dgrad through GELU: multiply by gelu'(h)
    h = _rand(M, N, seed=16).to(dtype)
    got = ops.gemm_t(d(A), d(W), act=2, aux_in=d(h))
    hh = h.double().requires_grad_(True)
    torch.nn.functional.gelu(hh, approximate="tanh").sum().backward()
    torch.testing.assert_close(got.cpu().double(), (A.double() @ W.double().t()) * hh.grad, **tol)
    # column sums of the output taken in the epilogue (bias gradient of the producing layer)
    cs = torch.full((N,), 2.0, device=DEV)
    got = ops.gemm_t(d(A), d(W), act=2, aux_in=d(h), colsum_out=cs, colsum_beta=0.5)
    torch.testing.assert_close(cs.cpu().double(), 1.0 + got.cpu().double().sum(0), rtol=1e-4, atol=1e-3)
    # wgrad with the bias gradient on the same launch: row sums of A^T (= column sums of the stored [K][M] operand)
    Xb, Yb = _mk(N, K, 4 * M, False, False, dtype, seed=19)
    rs = torch.full((N,), 3.0, device=DEV)
    got = ops.gemm_t(d(Xb), d(Yb), a_kmajor=False, b_kmajor=False, out_dtype=torch.float32, rowsum_a_out=rs, rowsum_a_beta=2.0)
    torch.testing.assert_close(got.cpu().double(), Xb.double().t() @ Yb.double(),
                               **(dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=1e-1)))
    torch.testing.assert_close(rs.cpu().double(), 6.0 + Xb.double().sum(0), rtol=1e-5, atol=1e-3)
    # wgrad accumulate: C = 1*C + A^T B
    X, Y = _mk(N, K, M, False, False, dtype, seed=17)
    c0 = _rand(N, K, seed=18)
    got = ops.gemm_t(d(X), d(Y), a_kmajor=False, b_kmajor=False, beta=1.0, out=d(c0).clone())
    torch.testing.assert_close(got.cpu().double(), c0.double() + X.double().t() @ Y.double(),
                               **(tol if dtype == torch.float32 else dict(rtol=2e-2, atol=5e-2)))


@pytest.mark.parametrize("tile", [10, 11, 13, 14])
@pytest.mark.parametrize("layout", ["fwd", "dgrad"])
def test_gemm_parked_drain_exact_integers(layout, tile):
    """(tiles 13 / 14: the same shapes on gemm_ws_kernel, the warp-specialised 128-row kernel -- 8 consumer + 4 loader waves.)
    gemm_pd_kernel (128-row tiles, the finished tile parked in registers and drained under the next tile's K loop): small
    integers are exact, so every element of every tile must match; shapes cover edge tiles in M and N, the shortest K it
    takes (12 K tiles: the unrolled drain K tiles and nothing else), an odd K tile count, one item per workgroup (everything
    drains in the open) and 3-4 items per workgroup (steady state), with fused column sums."""
    b_k = layout == "fwd"
    lib().vaw_debug_gemm_tile(tile)     # 10 / 11: the parked-drain kernel with 256 / 192 columns wherever it applies; 13 / 14: the warp-specialised one
    try:
        for (M, N, K) in [(256, 512, 768), (200, 72, 832), (1160, 776, 832), (16384, 768, 768), (40008, 520, 768), (20000, 3072, 960)]:
            A, B = _mk(M, N, K, True, b_k, torch.bfloat16, seed=M + N + K, ints=True)
            Ad, Bd = A.to(DEV), B.to(DEV)
            ref = _gemm_ref(A, B, True, b_k).float().bfloat16()
            cs = torch.zeros(N, device=DEV)
            got = ops.gemm_t(Ad, Bd, a_kmajor=True, b_kmajor=b_k, colsum_out=cs)
            assert torch.equal(got.cpu(), ref), (layout, tile, M, N, K, (got.cpu().double() - ref.double()).abs().max())
            torch.testing.assert_close(cs.cpu().double(), ref.double().sum(0), rtol=1e-6, atol=1e-2)
            got2 = ops.gemm_t(Ad, Bd, a_kmajor=True, b_kmajor=b_k)
            assert torch.equal(got2, got)
    finally:
        lib().vaw_debug_gemm_tile(-1)


@pytest.mark.parametrize("tile", [10, 11, 13, 14])
def test_gemm_parked_drain_epilogues_vs_persistent_kernel(tile):
    """The four epilogue kinds of the Linear launches on gemm_pd_kernel against gemm_p8_kernel on the same operands: bias + store,
    GELU with the saved pre-activation and the gated residual must be BITWISE equal (both round acc + bias to bf16 first);
    GELU' rounds the input gradient to bf16 before the multiply (the reference's autocast order), so it is held to one bf16 ulp
    of the persistent kernel and to the f64 reference within bf16 tolerance.  Edge rows, several items per workgroup."""
    Bt, T, D, H = 130, 64, 768, 3072
    M = Bt * T - 24                           # a ragged last row tile
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, D, generator=g).bfloat16().to(DEV)
    w1 = (torch.randn(H, D, generator=g) * 0.05).bfloat16().to(DEV)
    w2 = (torch.randn(D, H, generator=g) * 0.05).bfloat16().to(DEV)
    b1, b2 = torch.randn(H, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
    gate = torch.randn(Bt, D, generator=g).to(DEV)
    resid = torch.randn(M, D, generator=g).to(DEV)
    dy = torch.randn(M, D, generator=g).bfloat16().to(DEV)

    def run(t):
        lib().vaw_debug_gemm_tile(t)
        out = {}
        out["qkv"] = ops.gemm_t(x, w1[:2304].contiguous(), bias=b1[:2304].contiguous())
        a, hpre = ops.gemm_t(x, w1, bias=b1, act=1, want_aux=True)
        out["a"], out["hpre"] = a, hpre
        res = torch.empty(M, D, device=DEV)
        aux = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
        ops.gemm(BF16, 1, 1, M, D, H, ptr(a), H, ptr(w2), H, ptr(res), D, bias=ptr(b2), aux_out=ptr(aux), gate=ptr(gate), gate_ld=D,
                 resid=ptr(resid), rows_per_batch=T, out_f32=True)
        out["res"], out["y"] = res, aux
        cs = torch.zeros(H, device=DEV)
        out["dh"] = ops.gemm_t(dy, w2, b_kmajor=False, act=2, aux_in=hpre, colsum_out=cs)       # dy [M, D] . W2 [D, H] (as stored)
        out["dh_cs"] = cs
        cs2 = torch.zeros(D, device=DEV)
        out["dx"] = ops.gemm_t(out["dh"], w1, b_kmajor=False, colsum_out=cs2)
        out["dx_cs"] = cs2
        torch.cuda.synchronize()
        return out

    try:
        ref, got = run(3 if tile in (11, 14) else 2), run(tile)
    finally:
        lib().vaw_debug_gemm_tile(-1)
    for k in ("qkv", "a", "hpre", "res", "y"):
        assert torch.equal(ref[k], got[k]), (k, (ref[k].double() - got[k].double()).abs().max())
    # GELU': within one bf16 ulp of the single-rounding kernel, everywhere
    d = (ref["dh"].double() - got["dh"].double()).abs()
    assert bool((d <= ref["dh"].double().abs() * 2.0 ** -7 + 1e-30).all()), d.max()
    hh = got["hpre"].double().cpu().requires_grad_(True)
    torch.nn.functional.gelu(hh, approximate="tanh").sum().backward()
    exact = (dy.double().cpu() @ w2.double().cpu()) * hh.grad
    torch.testing.assert_close(got["dh"].double().cpu(), exact, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(got["dh_cs"].double().cpu(), got["dh"].double().sum(0).cpu(), rtol=1e-5, atol=1e-2)
    torch.testing.assert_close(got["dx_cs"].double().cpu(), got["dx"].double().sum(0).cpu(), rtol=1e-5, atol=1e-2)
    torch.testing.assert_close(got["dx"].double().cpu(), got["dh"].double().cpu() @ w1.double().cpu(), rtol=2e-2, atol=5e-2)


CANARY = 12345.5


def _colsum_partial_with_guard(rows, N):
    """A ColsumPartial whose buffer is the first `rows` rows of a larger tensor filled with a canary: writes past the capacity
    the caller stated land in the guard rows and are seen."""
    big = torch.full((rows + 64, N), CANARY, device=DEV)
    part = ops.ColsumPartial(1, N, torch.device(DEV))
    part.buf = big[:rows]
    return part, big


@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 13, 14])
@pytest.mark.parametrize("M", [2048, 4096, 16384])
def test_gemm_colsum_partial_each_path(tile, M):
    """vaw_gemm with colsum_partial_out on every dispatch target (vaw_debug_gemm_tile: 128 x 128, the 256 x 256 ring, the persistent
    kernel with 256 / 192 columns, the small-M ring kernels, the parked-drain kernel; -1 = by shape): the number of partial rows
    differs per kernel (one per 64, 128 or 256 rows of C), so each path must (a) report the rows it wrote, (b) write nothing beyond
    them -- guard rows behind the buffer keep their canary --, (c) fold to the column sums of C as stored, and (d) refuse, before
    anything is launched, a buffer one row too small (VAW_ERR_INVALID; C untouched).  Pins the round-3 fault: a 64-row kernel
    writing ceil(M/64) rows into a buffer sized for ceil(M/128)."""
    N, K = 768, 768
    A, B = _mk(M, N, K, True, False, torch.bfloat16, seed=M + 7)
    Ad, Bd = A.to(DEV), B.to(DEV)
    lib().vaw_debug_gemm_tile(tile)
    try:
        cap = (M + 63) // 64
        part, big = _colsum_partial_with_guard(cap, N)
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        ops.gemm(BF16, 1, 0, M, N, K, ptr(Ad), K, ptr(Bd), N, ptr(out), N, colsum_partial=part)
        torch.cuda.synchronize()
        R = part.rows.value
        assert 1 <= R <= cap, (tile, M, R)
        plan = ops.gemm_plan(BF16, 1, 0, M, N, K, ptr(Ad), K, ptr(Bd), N, ptr(out), N, colsum_partial_rows=cap,
                             workspace_floats=ops.scratch_f32(out.device, 0).numel())       # the workspace ops.gemm passed
        assert R == plan.colsum_rows, (tile, M, R, plan.colsum_rows, plan.variant)
        assert bool((big[R:] == CANARY).all()), (tile, M, R, "rows beyond the reported count were written")
        assert not bool((big[:R] == CANARY).any())
        torch.testing.assert_close(big[:R].double().sum(0).cpu(), out.double().sum(0).cpu(), rtol=1e-5, atol=2e-2)
        ref = (A.double() @ B.double()).float().bfloat16()
        torch.testing.assert_close(out.cpu().double(), ref.double(), rtol=2e-2, atol=2e-1)
        # one row short: an error, nothing launched
        part2, big2 = _colsum_partial_with_guard(R - 1, N) if R > 1 else (None, None)
        if part2 is not None:
            out2 = torch.full((M, N), 3.0, device=DEV, dtype=torch.bfloat16)
            with pytest.raises(vaw_amd.VawError, match="colsum_partial_out holds"):
                ops.gemm(BF16, 1, 0, M, N, K, ptr(Ad), K, ptr(Bd), N, ptr(out2), N, colsum_partial=part2)
            torch.cuda.synchronize()
            assert bool((big2 == CANARY).all()) and bool((out2 == 3.0).all())
    finally:
        lib().vaw_debug_gemm_tile(-1)


@pytest.mark.parametrize("B,H,T,hd", [(4, 12, 64, 64), (2, 4, 256, 64), (2, 4, 256, 96)])
@pytest.mark.parametrize("variant", ["0", "1", "2"])
def test_attn_bwd_colsum_capacity(B, H, T, hd, variant):
    """vaw_attn_bwd_colsum: rows written == *rows_out, guard rows untouched, and a buffer one row short is refused before the
    launch (every backward family: VAW_ATTN_BWD_BIG = 0 / 1 / 2 write B*T/64, B*T/256 or B*T/128 rows; T = 64: one per sample)."""
    os.environ["VAW_ATTN_BWD_BIG"] = variant
    try:
        D = H * hd
        qkv = (_rand(B * T, 3 * D, seed=T) * 0.7).bfloat16().to(DEV)
        do = _rand(B * T, D, seed=T + 1).bfloat16().to(DEV)
        o = torch.empty(B * T, D, device=DEV, dtype=torch.bfloat16)
        lse, delta = torch.empty(B * H * T, device=DEV), torch.empty(B * H * T, device=DEV)
        desc = ops.attn_desc_token_major(B, H, T, hd)
        ops.attn_fwd(BF16, desc, ptr(qkv), ptr(qkv) + 2 * D, ptr(qkv) + 4 * D, ptr(o), ptr(lse))
        args = (BF16, desc, ptr(qkv), ptr(qkv) + 2 * D, ptr(qkv) + 4 * D, ptr(o), ptr(do), ptr(lse), ptr(delta))
        dqkv = torch.zeros_like(qkv)
        part, big = _colsum_partial_with_guard(max(B, B * T // 64), 3 * D)
        assert ops.attn_bwd_colsum(*args, ptr(dqkv), ptr(dqkv) + 2 * D, ptr(dqkv) + 4 * D, part)
        torch.cuda.synchronize()
        R = part.rows.value
        assert bool((big[R:] == CANARY).all()) and not bool((big[:R] == CANARY).any())
        torch.testing.assert_close(big[:R].double().sum(0).cpu(), dqkv.double().sum(0).cpu(), rtol=1e-5, atol=2e-2)
        if R > 1:
            part2, big2 = _colsum_partial_with_guard(R - 1, 3 * D)
            dq2 = torch.full_like(qkv, 3.0)
            with pytest.raises(vaw_amd.VawError):
                ops.attn_bwd_colsum(*args, ptr(dq2), ptr(dq2) + 2 * D, ptr(dq2) + 4 * D, part2)
            torch.cuda.synchronize()
            assert bool((big2 == CANARY).all()) and bool((dq2 == 3.0).all())
    finally:
        os.environ.pop("VAW_ATTN_BWD_BIG", None)


@pytest.mark.parametrize("case", ["few_tiles_split", "full_rounds_plus_split", "n192", "edges_accumulate"])
def test_wgrad_grouped_exact_integers(case):
    """vaw_wgrad_grouped: many dW_p (+)= dy_p^T x_p in one launch; whole tiles + K-split tiles of the last round + fixup.
    Small integers are exact in bf16 / f32, so every tile of every problem must match bit for bit."""
    g = torch.Generator().manual_seed(11)
    shapes, K, beta = {
        "few_tiles_split": ([(768, 768), (2304, 768), (256, 512)], 1024, 0.0),            # 9 + 27 + 2 tiles: all K-split
        "full_rounds_plus_split": ([(512, 512)] * 70, 2560, 0.0),                          # 280 tiles: 256 whole + 24 split
        "n192": ([(384, 1152), (1152, 384), (256, 192)], 512, 0.0),                        # every N % 192 == 0: 192-column tiles
        "edges_accumulate": ([(200, 264), (520, 72), (136, 1000)], 320, 1.0),              # edge tiles in M and N, beta = 1
    }[case]
    probs, keep, refs = [], [], []
    for (M, N) in shapes:
        dy = torch.randint(-2, 3, (K, M), generator=g).float()
        x = torch.randint(-2, 3, (K, N), generator=g).float()
        dw0 = torch.randint(-5, 6, (M, N), generator=g).float()
        dyd, xd, dwd = dy.to(DEV).bfloat16(), x.to(DEV).bfloat16(), dw0.to(DEV).clone()
        keep += [dyd, xd, dwd]
        probs.append((ptr(dyd), ptr(xd), ptr(dwd), M, N, M, N, N))
        refs.append((dwd, beta * dw0.double() + dy.double().t() @ x.double()))
    grp = ops.WgradGroup(probs, K, torch.device(DEV))
    grp.launch(BF16, beta)
    for i, (got, ref) in enumerate(refs):
        assert torch.equal(got.cpu().double(), ref), (case, i, shapes[i], (got.cpu().double() - ref).abs().max())
    if beta == 0.0:      # second launch reuses the uploaded table and must reproduce the result
        grp.launch(BF16, 0.0)
        for got, ref in refs:
            assert torch.equal(got.cpu().double(), ref)


@pytest.mark.parametrize("M,tile", [(2048, 0), (8192, 4)])
@pytest.mark.parametrize("layout", ["fwd", "dgrad"])
def test_gemm_small_m_long_k_bf16_split_exact_integers(layout, M, tile):
    """The strong-scaling shapes (few output tiles, long K, plain bf16 result) take a K-split path -- of the 128 x 128 kernel at
    2048 rows, of the persistent kernel (half-full launch) at 8192: f32 slabs + a fixed-order reduce that writes bf16.  Small
    integers: exact, and identical on a repeat."""
    N, K = 768, 3072
    g = torch.Generator().manual_seed(5)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    B = torch.randint(-2, 3, (N, K) if layout == "fwd" else (K, N), generator=g).float()
    ref = (A.double() @ (B.double().t() if layout == "fwd" else B.double())).float().bfloat16()
    Ad, Bd = A.to(DEV).bfloat16(), B.to(DEV).bfloat16()
    lib().vaw_debug_gemm_tile(tile)       # 0: the 128 x 128 kernel (what the planner picks at 2048 rows), 4: the persistent one
    try:
        out = ops.gemm_t(Ad, Bd, a_kmajor=True, b_kmajor=layout == "fwd")
        out2 = ops.gemm_t(Ad, Bd, a_kmajor=True, b_kmajor=layout == "fwd")
    finally:
        lib().vaw_debug_gemm_tile(-1)
    assert torch.equal(out.cpu(), ref) and torch.equal(out, out2)


def test_gemm_rejects_bad_arguments():
    A = torch.zeros(8, 8, device=DEV)
    with pytest.raises(vaw_amd.VawError):
        ops.gemm(F32, 1, 1, 8, 8, 8, ptr(A), 4, ptr(A), 8, ptr(A), 8)          # lda < K
    with pytest.raises(vaw_amd.VawError):
        ops.gemm(F32, 1, 1, 8, 8, 8, ptr(A), 8, ptr(A), 8, ptr(A), 8, act=2)   # act=2 without aux_in
    with pytest.raises(vaw_amd.VawError):
        ops.qsample(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), torch.zeros(10), torch.zeros(10))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum(dtype):
    for (M, N) in [(1000, 260), (3, 8), (2048, 768)]:
        X = _rand(M, N, seed=M).to(dtype)
        out = _rand(N, seed=1).to(DEV)
        o0 = out.clone()
        ops.colsum(ops.dt_of(X), ptr(X.to(DEV)), M, N, N, ptr(out), 0.0)
        torch.testing.assert_close(out.cpu().double(), X.double().sum(0), rtol=1e-5, atol=1e-3)
        out = o0.clone()
        Xd = X.to(DEV)
        ops.colsum(ops.dt_of(X), ptr(Xd), M, N, N, ptr(out), 1.0)
        torch.testing.assert_close(out.cpu().double(), o0.cpu().double() + X.double().sum(0), rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------------
# LayerNorm + modulate, gated residual backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,D", [(3, 16, 64), (2, 64, 768), (2, 5, 1152), (1, 1, 8)])
def test_ln_modulate_fwd_bwd(dtype, B, T, D):
    tol = dict(rtol=1e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    x = _rand(B * T, D, seed=1) * 2 + 0.5
    mod = _rand(B, 6 * D, seed=2) * 0.5
    dout = _rand(B * T, D, seed=3).to(dtype)
    dres = _rand(B * T, D, seed=4)
    xr = x.double().requires_grad_(True)
    modr = mod.double().requires_grad_(True)
    shift, scale = modr[:, 3 * D:4 * D], modr[:, 4 * D:5 * D]
    ref = torch.nn.functional.layer_norm(xr, (D,), eps=1e-6).view(B, T, D) * (1 + scale[:, None]) + shift[:, None]
    (ref.reshape(B * T, D) * dout.double()).sum().backward()
    xd, md = x.to(DEV), mod.to(DEV)
    out = torch.empty(B * T, D, device=DEV, dtype=dtype)
    mean, rstd = torch.empty(B * T, device=DEV), torch.empty(B * T, device=DEV)
    dt = ops.dt_of(out)
    ops.ln_modulate_fwd(dt, ptr(xd), ptr(md) + 4 * 3 * D, ptr(md) + 4 * 4 * D, 6 * D, ptr(out), ptr(mean), ptr(rstd), B, T, D)
    torch.testing.assert_close(out.cpu().double(), ref.detach().reshape(B * T, D), **tol)
    torch.testing.assert_close(mean.cpu().double(), x.double().mean(1), rtol=1e-5, atol=1e-6)
    dmod = torch.zeros(B, 6 * D, device=DEV)
    dx = dres.to(DEV).clone()
    dod = dout.to(DEV)
    ops.ln_modulate_bwd(dt, ptr(dod), ptr(xd), ptr(mean), ptr(rstd), ptr(md) + 4 * 4 * D, 6 * D, ptr(dx), ptr(dx),
                        ptr(dmod) + 4 * 3 * D, ptr(dmod) + 4 * 4 * D, 6 * D, B, T, D)
    torch.testing.assert_close(dx.cpu().double(), dres.double() + xr.grad, **tol)
    torch.testing.assert_close(dmod.cpu().double(), modr.grad, rtol=tol["rtol"], atol=tol["atol"] * math.sqrt(T))
    # no incoming residual gradient
    dx2 = torch.empty(B * T, D, device=DEV)
    ops.ln_modulate_bwd(dt, ptr(dod), ptr(xd), ptr(mean), ptr(rstd), ptr(md) + 4 * 4 * D, 6 * D, 0, ptr(dx2),
                        ptr(dmod) + 4 * 3 * D, ptr(dmod) + 4 * 4 * D, 6 * D, B, T, D)
    torch.testing.assert_close(dx2.cpu().double(), xr.grad, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_bwd(dtype):
    B, T, D = 3, 20, 192
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    dres, y, gate = _rand(B * T, D, seed=1), _rand(B * T, D, seed=2).to(dtype), _rand(B, 2 * D, seed=3)
    dy = torch.empty(B * T, D, device=DEV, dtype=dtype)
    dg = torch.zeros(B, 2 * D, device=DEV)
    gd, dr, yd = gate.to(DEV), dres.to(DEV), y.to(DEV)
    ops.gate_bwd(ops.dt_of(dy), ptr(dr), ptr(yd), ptr(gd) + 4 * D, 2 * D, ptr(dy), ptr(dg) + 4 * D, 2 * D, B, T, D)
    g = gate[:, D:].double()
    torch.testing.assert_close(dy.cpu().double(), dres.double() * g.repeat_interleave(T, 0), **tol)
    torch.testing.assert_close(dg[:, D:].cpu().double(), (dres.double() * y.double()).view(B, T, D).sum(1), rtol=1e-4, atol=1e-4)
    assert float(dg[:, :D].abs().max()) == 0.0
    # bias-gradient partials: per-sample column sums of dy as stored, then the fixed-order reduce over samples
    part = torch.empty(B, D, device=DEV)
    ops.gate_bwd(ops.dt_of(dy), ptr(dr), ptr(yd), ptr(gd) + 4 * D, 2 * D, ptr(dy), ptr(dg) + 4 * D, 2 * D, B, T, D, ptr(part))
    torch.testing.assert_close(part.cpu().double(), dy.cpu().double().view(B, T, D).sum(1), rtol=1e-5, atol=1e-5)
    out = torch.ones(D, device=DEV)
    ops.reduce_rows(ptr(part), B, D, ptr(out), 1.0)
    torch.testing.assert_close(out.cpu().double(), 1.0 + dy.cpu().double().sum(0), rtol=1e-5, atol=1e-4)


# DiT-L/2 and DiT-XL/2 at their per-GPU batches: the fused entry aims at 512 workgroups there, so the pair must cut rows the same way;
# D = 1216 / 1280 at 8 waves: the fused pass's LDS slabs do not fit, it runs the register form
FUSED_PAIR_SHAPES = [(3, 16, 64), (2, 64, 768), (2, 24, 1152), (300, 8, 192), (2, 24, 1216), (2, 100, 1280), (3, 5, 1280),
                     (2, 40, 260), (2, 40, 1028), (32, 256, 1024), (128, 256, 1152)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,D", FUSED_PAIR_SHAPES)
def test_ln_modulate_bwd_fused_with_gate_bwd_is_bitwise_the_pair(dtype, B, T, D):
    """vaw_ln_modulate_bwd_gate = vaw_ln_modulate_bwd followed by vaw_gate_bwd on its dx, one pass: every output bitwise equal
    (B = 2, 3: rows split over several workgroups + fold launch; B = 300: one workgroup per sample)."""
    _fused_vs_pair(dtype, B, T, D, alias=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,D", FUSED_PAIR_SHAPES[:9])
def test_ln_modulate_bwd_fused_with_gate_bwd_in_place_is_bitwise_the_pair(dtype, B, T, D):
    """As above with dres_in == dx, the way dit.py calls both (the residual-stream gradient accumulates in place)."""
    _fused_vs_pair(dtype, B, T, D, alias=True)


def _fused_vs_pair(dtype, B, T, D, alias):
    x = (_rand(B * T, D, seed=1) * 2 + 0.5).to(DEV)
    mod = (_rand(B, 6 * D, seed=2) * 0.5).to(DEV)
    dout = _rand(B * T, D, seed=3).to(dtype).to(DEV)
    dres = _rand(B * T, D, seed=4).to(DEV)
    y = _rand(B * T, D, seed=5).to(dtype).to(DEV)
    mean, rstd = torch.empty(B * T, device=DEV), torch.empty(B * T, device=DEV)
    out = torch.empty(B * T, D, device=DEV, dtype=dtype)
    dt = ops.dt_of(out)
    ops.ln_modulate_fwd(dt, ptr(x), ptr(mod) + 4 * 3 * D, ptr(mod) + 4 * 4 * D, 6 * D, ptr(out), ptr(mean), ptr(rstd), B, T, D)

    def run(fused):
        dmod = torch.zeros(B, 6 * D, device=DEV)
        dx, dy, part = torch.empty(B * T, D, device=DEV), torch.empty(B * T, D, device=DEV, dtype=dtype), torch.empty(B, D, device=DEV)
        if alias:
            dx.copy_(dres)
        a = (dt, ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(mod) + 4 * 4 * D, 6 * D, ptr(dx) if alias else ptr(dres), ptr(dx),
             ptr(dmod) + 4 * 3 * D, ptr(dmod) + 4 * 4 * D, 6 * D)
        if fused:       # the C entry point itself (ops.ln_modulate_bwd_gate sends rows wider than 1280 to the pair)
            ws = ops._row_ws(B, T, D)
            ops.check(lib().vaw_ln_modulate_bwd_gate(*a, ptr(y), ptr(mod) + 4 * 5 * D, ptr(dy), ptr(dmod) + 4 * 5 * D, ptr(part), B, T, D,
                                                     ws.data_ptr(), ws.numel(), stream_ptr()), "vaw_ln_modulate_bwd_gate")
        else:
            ops.ln_modulate_bwd(*a, B, T, D)
            ops.gate_bwd(dt, ptr(dx), ptr(y), ptr(mod) + 4 * 5 * D, 6 * D, ptr(dy), ptr(dmod) + 4 * 5 * D, 6 * D, B, T, D, ptr(part))
        torch.cuda.synchronize()
        return dx, dy, dmod, part
    for u, f in zip(run(False), run(True)):
        assert torch.equal(u, f)


def test_reduce_rows_batched_is_bitwise_reduce_rows():
    """One launch for many (partial rows -> column sums) folds, each with vaw_reduce_rows' summation tree."""
    shapes = [(256, 768), (128, 3072), (1, 2304), (37, 40), (300, 8), (33, 1000)]
    parts = [(_rand(R, N, seed=10 + i) * 3).to(DEV) for i, (R, N) in enumerate(shapes)]
    for beta in (0.0, 1.0):
        ref = [(_rand(N, seed=50 + i)).to(DEV) for i, (R, N) in enumerate(shapes)]
        got = [r.clone() for r in ref]
        for p_, r_ in zip(parts, ref):
            ops.reduce_rows(ptr(p_), p_.shape[0], p_.shape[1], ptr(r_), beta)
        grp = ops.ReduceGroup([(ptr(p_), ptr(g_), p_.shape[0], p_.shape[1]) for p_, g_ in zip(parts, got)], torch.device(DEV))
        grp.launch(beta)
        torch.cuda.synchronize()
        for r_, g_, p_ in zip(ref, got, parts):
            assert torch.equal(r_, g_)
            if beta == 0.0:
                torch.testing.assert_close(g_.cpu().double(), p_.cpu().double().sum(0), rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------
# attention: both memory layouts, forward + backward
# ------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, scale):
    """q,k,v [B,H,T,hd] float64"""
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    return p @ v


@pytest.mark.parametrize("dtype,rowwise", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False)])
@pytest.mark.parametrize("B,H,T,hd", [(2, 3, 64, 64), (1, 2, 16, 32), (2, 2, 100, 72), (1, 1, 256, 64), (3, 2, 128, 64),
                                      (2, 4, 256, 96), (1, 2, 1024, 64), (2, 2, 64, 32), (1, 2, 192, 128),
                                      (2, 3, 128, 72), (1, 3, 64, 40), (1, 16, 256, 72)])
def test_attention_token_major(dtype, rowwise, B, H, T, hd):
    """rowwise=False lets bf16 / hd % 8 == 0 / T % 64 == 0 shapes take the MFMA kernels (head dims such as DiT-XL's 72
    are zero-padded to 96 in LDS and must not spill into the neighbouring head); the others always run rowwise."""
    tol = dict(rtol=1e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    lib().vaw_debug_force_rowwise_attention(1 if rowwise else 0)
    _forced_rowwise[0] = bool(rowwise)
    try:
        _attention_token_major(dtype, tol, B, H, T, hd)
    finally:
        lib().vaw_debug_force_rowwise_attention(0)
        _forced_rowwise[0] = False


def _attention_token_major(dtype, tol, B, H, T, hd):
    D = H * hd
    qkv = (_rand(B * T, 3 * D, seed=T) * 0.7).to(dtype)
    do = _rand(B * T, D, seed=T + 1).to(dtype)
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)
    ref = _attn_ref(q, k, v, hd ** -0.5).transpose(1, 2).reshape(B * T, D)
    (ref * do.double()).sum().backward()
    qd, dod = qkv.to(DEV), do.to(DEV)
    o = torch.empty(B * T, D, device=DEV, dtype=dtype)
    lse, delta = torch.empty(B * H * T, device=DEV), torch.empty(B * H * T, device=DEV)
    dt, es = ops.dt_of(o), qkv.element_size()
    desc = ops.attn_desc_token_major(B, H, T, hd)
    ops.attn_fwd(dt, desc, ptr(qd), ptr(qd) + es * D, ptr(qd) + 2 * es * D, ptr(o), ptr(lse))
    torch.testing.assert_close(o.cpu().double(), ref.detach(), **tol)
    dqkv = torch.zeros_like(qd)
    ops.attn_bwd(dt, desc, ptr(qd), ptr(qd) + es * D, ptr(qd) + 2 * es * D, ptr(o), ptr(dod), ptr(lse), ptr(delta),
                 ptr(dqkv), ptr(dqkv) + es * D, ptr(dqkv) + 2 * es * D)
    torch.testing.assert_close(dqkv.cpu().double(), qr.grad, **tol)
    # the same backward with the column sums of dq | dk | dv as partial rows (the qkv bias gradient): MFMA kernels only
    part = ops.ColsumPartial(max(B, B * T // 64), 3 * D, torch.device(DEV))
    dqkv2 = torch.zeros_like(qd)
    took = ops.attn_bwd_colsum(dt, desc, ptr(qd), ptr(qd) + es * D, ptr(qd) + 2 * es * D, ptr(o), ptr(dod), ptr(lse), ptr(delta),
                               ptr(dqkv2), ptr(dqkv2) + es * D, ptr(dqkv2) + 2 * es * D, part)
    mfma = dtype == torch.bfloat16 and T % 64 == 0 and hd % 8 == 0 and not lib_forced_rowwise()
    assert took == mfma
    if took:
        assert torch.equal(dqkv2, dqkv)
        R = part.rows.value
        wgr = {"0": 0, "1": 256, "2": 128}[os.environ.get("VAW_ATTN_BWD_BIG", "2")]       # attention_bwd_big.hip: one row per workgroup of 256 / 128 owner rows
        big = wgr and T % wgr == 0 and T <= 1024 and 32 < hd <= 96
        assert R == (B if T == 64 else B * (T // wgr) if big else B * (T // 64) // (2 if (T % 128 == 0 and 64 < hd <= 96) else 1))
        torch.testing.assert_close(part.buf[:R].sum(0).cpu().double(), dqkv.cpu().double().sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("variant", ["0", "1"])
@pytest.mark.parametrize("B,H,T,hd", [(1, 1, 256, 64), (2, 4, 256, 96), (1, 2, 1024, 64), (1, 16, 256, 72), (2, 2, 512, 40), (3, 2, 128, 64)])
def test_attention_backward_other_variants(B, H, T, hd, variant):
    """VAW_ATTN_BWD_BIG=0 / 1: the 16-row backward kernels and the 64-rows-per-wave pair (the default for these shapes is the
    32-rows-per-wave pair of attention_bwd_big.hip, which test_attention_token_major runs) give the same gradients and column sums
    as the reference within the bf16 tolerance."""
    os.environ["VAW_ATTN_BWD_BIG"] = variant
    os.environ["VAW_ATTN_FWD_BIG"] = "1" if variant == "0" else "0"      # (and the forward's two forms, crossed with the backward's)
    try:
        _attention_token_major(torch.bfloat16, dict(rtol=3e-2, atol=3e-2), B, H, T, hd)
    finally:
        del os.environ["VAW_ATTN_BWD_BIG"]
        del os.environ["VAW_ATTN_FWD_BIG"]


_forced_rowwise = [False]


def lib_forced_rowwise():
    return _forced_rowwise[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_channel_major_unet_layout(dtype):
    """UNet QKVAttention (new order): qkv [B, 3*H*ch, T]; scale ch^-1/4 on q and on k == ch^-1/2 on the product."""
    from oracle.unet import QKVAttention
    B, H, T, ch = 2, 4, 64, 32
    tol = dict(rtol=1e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    qkv = (_rand(B, 3 * H * ch, T, seed=5) * 0.8).to(dtype)
    do = _rand(B, H * ch, T, seed=6).to(dtype)
    qr = qkv.double().requires_grad_(True)
    ref = QKVAttention(H)(qr)
    (ref * do.double()).sum().backward()
    qd, dod = qkv.to(DEV), do.to(DEV)
    o = torch.empty(B, H * ch, T, device=DEV, dtype=dtype)
    lse, delta = torch.empty(B * H * T, device=DEV), torch.empty(B * H * T, device=DEV)
    dt, es = ops.dt_of(o), qkv.element_size()
    desc = ops.attn_desc_channel_major(B, H, T, ch)
    koff, voff = es * H * ch * T, 2 * es * H * ch * T
    ops.attn_fwd(dt, desc, ptr(qd), ptr(qd) + koff, ptr(qd) + voff, ptr(o), ptr(lse))
    torch.testing.assert_close(o.cpu().double(), ref.detach(), **tol)
    dqkv = torch.zeros_like(qd)
    ops.attn_bwd(dt, desc, ptr(qd), ptr(qd) + koff, ptr(qd) + voff, ptr(o), ptr(dod), ptr(lse), ptr(delta), ptr(dqkv),
                 ptr(dqkv) + koff, ptr(dqkv) + voff)
    torch.testing.assert_close(dqkv.cpu().double(), qr.grad, **tol)


# ------------------------------------------------------------------------------------------------
# small conditioning kernels, patch shuffles
# ------------------------------------------------------------------------------------------------
def test_timestep_embedding_vs_golden():
    g = load_pt("unet_tiny.pt")
    t = g["temb/t"].to(DEV)
    torch.testing.assert_close(ops.timestep_embedding(t, 64).cpu(), g["temb/out64"], rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(ops.timestep_embedding(t, 33).cpu(), g["temb/out33"], rtol=1e-5, atol=2e-6)


def test_patchify_unpatchify_roundtrip_and_order():
    B, C, H, p = 3, 4, 16, 4
    x = _rand(B, C, H, H, seed=1)
    xd = x.to(DEV)
    tok = torch.empty(B * (H // p) ** 2, C * p * p, device=DEV)
    st = stream_ptr()
    assert lib().vaw_patchify(F32, ptr(xd), ptr(tok), B, C, H, H, p, st) == 0
    ref = torch.nn.functional.unfold(x, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, C * p * p)   # (c,i,j) order
    assert torch.equal(tok.cpu(), ref)
    back = torch.empty_like(xd)
    assert lib().vaw_patchify_bwd(ptr(tok), ptr(back), B, C, H, H, p, st) == 0
    assert torch.equal(back.cpu(), x)
    # final-layer order (i,j,c): oracle unpatchify
    from oracle.dit import DiT
    m = DiT(image_size=H, patch_size=p, in_channels=C, hidden_size=32, depth=1, num_heads=2, num_classes=3)
    tk = _rand(B, (H // p) ** 2, p * p * C, seed=2)
    img = torch.empty(B, C, H, H, device=DEV)
    tkd = tk.to(DEV).reshape(-1, p * p * C).contiguous()
    assert lib().vaw_unpatchify(F32, ptr(tkd), ptr(img), B, C, H, H, p, st) == 0
    assert torch.equal(img.cpu(), m.unpatchify(tk))
    tk2 = torch.empty_like(tkd)
    assert lib().vaw_unpatchify_bwd(F32, ptr(img), ptr(tk2), B, C, H, H, p, st) == 0
    assert torch.equal(tk2, tkd)


# ------------------------------------------------------------------------------------------------
# optimizer kernels
# ------------------------------------------------------------------------------------------------
def test_fused_adamw_ema_matches_torch_adamw():
    n = 10007
    p0, = [_rand(n, seed=1)]
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref_p], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    ema_ref = p0.clone()
    p, m, v, e = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(DEV).clone()
    shadow = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(1, device=DEV)
    for step in range(1, 6):
        g = _rand(n, seed=10 + step) * (3.0 if step == 3 else 0.1)
        ref_p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        ema_ref = ema_ref * 0.999 + ref_p.detach() * (1 - 0.999)
        gd = g.to(DEV)
        ops.sumsq(gd, ss)
        torch.testing.assert_close(ss.cpu().double(), (g.double() ** 2).sum().view(1), rtol=1e-5, atol=0)
        ops.adamw_ema_step(p, gd, m, v, e, shadow, 1e-3, 0.9, 0.95, 1e-8, 0.01, step, 0.999, ss, 1.0, True)
        assert float(gd.abs().max()) == 0.0
    torch.testing.assert_close(p.cpu(), ref_p.detach(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(e.cpu(), ema_ref, rtol=1e-6, atol=1e-7)
    assert torch.equal(shadow.cpu(), p.cpu().bfloat16())

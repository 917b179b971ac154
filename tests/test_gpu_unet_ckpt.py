"""Activation recomputation of the HIP UNet (UNetModel(use_checkpoint=True) / set_activation_checkpointing): every ResBlock and
AttentionBlock is re-run in backward from its input, on the GroupNorm statistics and the packed dropout bits of the first forward.
The flag changes no bit of the output or of any gradient, and lowers the peak memory of a step.  Also the two kernels the
recomputation adds, through their C entry points: vaw_groupnorm_apply against vaw_groupnorm_fwd, the packed dropout against vaw_mul."""
import copy
import random

import numpy as np
import pytest
import torch

from conftest import Pbar, base_args, load_json, perturb_, synth_loader

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, GN_APPLY, GN_FWD_SUMS, GNV_FLAT, GNV_QUAD, lib, ptr, stream_ptr

DEV = "cuda"
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}


def _model(dtype, ckpt, ssn=True, updown=True, new_order=True, dropout=0.0, size=16, ch=32, nres=1, att="8"):
    torch.manual_seed(21)
    m = vaw_amd.create_unet_model(image_size=size, num_channels=ch, num_res_blocks=nres, channel_mult="1,2", attention_resolutions=att,
                                  num_heads=2, use_scale_shift_norm=ssn, resblock_updown=updown, use_new_attention_order=new_order,
                                  dropout=dropout, use_checkpoint=ckpt, compute_dtype=dtype)
    assert m.activation_checkpointing is bool(ckpt)
    m = m.to(DEV).train()
    perturb_(m, 77, std=0.03)          # the zero-initialised convs would cut every gradient path
    return m


def _inputs(B, size, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, size, size, generator=g).to(DEV), (torch.rand(B, generator=g) * 999).to(DEV),
            torch.randint(0, 10, (B,), generator=g).to(DEV), torch.randn(B, 3, size, size, generator=g).to(DEV))


def _step(m, x, t, y, gout, micro=1, need_dx=True, between=None):
    """`micro` forward / backward pairs (the second accumulates: beta = 1) -> outputs, dx, parameter gradients."""
    outs, dxs = [], []
    for i in range(micro):
        xr = (x + 0.1 * i).clone().requires_grad_(need_dx)
        out = m(xr, t, y=y)
        if between is not None:
            between()
        (out * gout).sum().backward()
        outs.append(out.detach().clone())
        dxs.append(xr.grad.clone() if need_dx else None)
    return outs, dxs, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _assert_same(a, b, what):
    (oa, xa, ga), (ob, xb, gb) = a, b
    for i, (u, v) in enumerate(zip(oa, ob)):
        assert torch.equal(u, v), f"{what}: output of micro-step {i}"
    for i, (u, v) in enumerate(zip(xa, xb)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: dx of micro-step {i}"
    assert set(ga) == set(gb) and len(ga) > 20
    for k in ga:
        assert torch.equal(ga[k], gb[k]), f"{what}: gradient of {k}"
        assert float(ga[k].abs().max()) > 0 or not k.endswith("weight"), f"{what}: {k} got no gradient"


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ssn", [True, False])
@pytest.mark.parametrize("updown", [True, False])
@pytest.mark.parametrize("new_order", [True, False])
def test_flag_changes_no_bit(dtype, ssn, updown, new_order):
    """Output, dx and EVERY parameter gradient with use_checkpoint=True are bitwise those of the same weights with the flag off:
    one micro-step (beta = 0) and a two-micro-step accumulation (beta = 1)."""
    x, t, y, gout = _inputs(2, 16)
    for micro in (1, 2):
        ref = _step(_model(dtype, False, ssn, updown, new_order), x, t, y, gout, micro)
        got = _step(_model(dtype, True, ssn, updown, new_order), x, t, y, gout, micro)
        _assert_same(got, ref, f"{dtype} ssn={ssn} updown={updown} new_order={new_order} micro={micro}")


def _peak_of_step(m, x, t, y, gout, need_dx=False):
    """Peak of torch.cuda.max_memory_allocated over one forward + backward, above what is allocated before it (weights, gradients,
    the reduction scratch: the step before has allocated whatever is allocated once)."""
    _step(m, x, t, y, gout, need_dx=need_dx)          # (the measured step accumulates onto this one's gradients: beta = 1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = _step(m, x, t, y, gout, need_dx=need_dx)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, res


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("host_rng", [False, True])
def test_dropout_masks_are_replayed_not_redrawn(dtype, host_rng):
    """dropout = 0.1: the recomputation replays the first forward's mask from its bits, so with the same seed the flag changes no
    bit and leaves the generator (device, or CPU with host_dropout_rng) where the flag-off run leaves it.  The flag must also DO
    something: the step's peak memory drops."""
    x, t, y, gout = _inputs(2, 16)
    res, peak, state = {}, {}, {}
    for ckpt in (False, True):
        m = _model(dtype, ckpt, dropout=0.1)
        m.host_dropout_rng = host_rng
        torch.manual_seed(5)
        peak[ckpt], res[ckpt] = _peak_of_step(m, x, t, y, gout)
        state[ckpt] = torch.get_rng_state() if host_rng else torch.cuda.get_rng_state()
    _assert_same(res[True], res[False], f"dropout {dtype} host_rng={host_rng}")
    assert torch.equal(state[True], state[False]), "the generator moved differently with the flag on"
    print(f"dropout model {dtype}: peak above baseline off {peak[False]} on {peak[True]} bytes")
    assert peak[True] < peak[False]


def _unit_intermediate_bytes(m, B, size, es):
    """Per ResBlock / AttentionBlock, in forward order: the bytes of the tensors the plain tape keeps alive until backward and a
    checkpointed unit does not (everything between the unit's input and its output), by hand from the topology."""
    from vaw_amd.unet import AttentionBlock, ResBlock
    out, H = [], size
    for layer in [l for blk in list(m.input_blocks) + [m.middle_block] + list(m.output_blocks) for l in blk]:
        if isinstance(layer, ResBlock):
            M, Ci, Co = B * H * H, layer.channels, layer.out_channels
            n = M * Ci                                           # GroupNorm + SiLU of the input
            if layer.updown:
                H = H * 2 if layer.up else H // 2
                M = B * H * H
                n += 2 * M * Ci                                  # resampled h and x
            n += 2 * M * Co                                      # first conv, second GroupNorm
            if Ci != Co:
                n += M * Co                                      # 1 x 1 skip connection
            out.append(es * n)
        elif isinstance(layer, AttentionBlock):
            M, C = B * H * H, layer.channels
            out.append(es * 5 * M * C + 4 * B * layer.num_heads * H * H)      # norm, qkv (3 C), attention output; lse
    return out


def test_peak_memory_drops():
    """Depth num_res_blocks = 3, batch 8, 32 x 32, 64 channels, bf16: the peak of a forward + backward with the flag on is below
    the flag-off peak.  Without the feature both peaks are equal.

    The bound.  The issue asks for `on <= off - 0.5 x (off - on_measured)` with both peaks measured once on a card.  NO CARD RUN
    COULD BE MADE when this was written, so the saving is predicted instead, from the shapes alone and not from what the
    code gives: with I_u the bytes a unit's plain tape holds between its input and its output (_unit_intermediate_bytes), the
    flag-off step holds sum(I_u) when backward starts, the flag-on step holds one unit's I_u at a time, so the saving is
    sum(I_u) - max(I_u) less the recomputed output and the statistics a checkpointed unit adds; half of it is asserted, the issue's
    margin.  Replace the prediction by the two measured peaks when a card has run this test."""
    x, t, y, gout = _inputs(8, 32)
    peak = {}
    for ckpt in (False, True):
        m = _model("bf16", ckpt, size=32, ch=64, nres=3, att="16")
        peak[ckpt], _ = _peak_of_step(m, x, t, y, gout)
        units = _unit_intermediate_bytes(m, 8, 32, 2)
        del m
    off, on = peak[False], peak[True]
    predicted = sum(units) - max(units)
    print(f"depth-3 model: peak above baseline off {off} on {on} bytes, ratio {on / off:.4f}; {len(units)} units, predicted saving {predicted}")
    assert len(units) == 26 and predicted > 64 << 20          # 78.1 MiB in all, the largest unit 8.5 MiB
    assert on < off
    assert on <= off - 0.5 * predicted


# ---- vaw_groupnorm_apply ------------------------------------------------------------------------------------------------------
def _gn_case(dt, B, HW, C, film, silu, seed):
    g = torch.Generator().manual_seed(seed)
    td = TORCH_DT[dt]
    x = (torch.randn(B * HW, C, generator=g) * 1.5 + 0.3).to(DEV, td)
    gam, bet = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    tab = (torch.randn(B, 3 * C, generator=g) * 0.3).to(DEV)          # FiLM rows with a stride wider than 2 C, as in the engine
    sc, sh = (ptr(tab), ptr(tab) + 4 * C) if film else (None, None)
    y0 = torch.full((B * HW + 8, C), 7.0, device=DEV, dtype=td)          # 8 canary rows behind each output
    y1 = torch.full((B * HW + 8, C), 7.0, device=DEV, dtype=td)
    mean, rstd = torch.empty(B * 32, device=DEV), torch.empty(B * 32, device=DEV)
    ws = torch.empty(lib().vaw_groupnorm_workspace_floats(B, HW, C), device=DEV)
    assert lib().vaw_groupnorm_fwd(dt, ptr(x), ptr(gam), ptr(bet), sc, sh, 3 * C, int(silu), ptr(y0), ptr(mean), ptr(rstd), B, HW, C, 32,
                                   1e-5, ptr(ws), stream_ptr()) == 0
    assert lib().vaw_groupnorm_apply(dt, ptr(x), ptr(mean), ptr(rstd), ptr(gam), ptr(bet), sc, sh, 3 * C, int(silu), ptr(y1), B, HW, C, 32,
                                     stream_ptr()) == 0
    what = f"dt={dt} B={B} HW={HW} C={C} film={film} silu={silu}"
    assert torch.equal(y0, y1), what
    assert bool((y1[B * HW:] == 7.0).all()) and bool(torch.isfinite(y1.float()).all()), what
    assert float(y1[:B * HW].float().std()) > 0.05, what


@pytest.mark.parametrize("film", [True, False])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("path", ["f32_quad", "bf16_quad", "bf16_flat_forced", "bf16_flat_by_shape"])
def test_groupnorm_apply_is_the_forward_apply_pass(path, film, silu):
    """vaw_groupnorm_apply on the statistics vaw_groupnorm_fwd wrote = vaw_groupnorm_fwd's output, bitwise, on every dispatch
    path of the apply pass; ops.gn_plan says that each `path` is the variant its name names.  The small shapes are flat only when
    forced through vaw_debug_gn_flat(1) (128-row chunks: HW = 16 and 64 are a short single chunk, HW = 1024 is 8 chunks); B = 128,
    HW = 512 is flat by shape (4 chunks x 128 samples)."""
    dt = F32 if path == "f32_quad" else BF16
    shapes = [(B, HW, C) for C in (32, 96, 192) for HW in (16, 64, 1024) for B in (1, 3)]
    if path == "bf16_flat_by_shape":
        shapes = [(128, 512, 32), (128, 512, 96)]
    try:
        if path == "bf16_flat_forced":
            lib().vaw_debug_gn_flat(1)
        for i, (B, HW, C) in enumerate(shapes):
            assert all(ops.gn_plan(p, dt, B, HW, C).variant == (GNV_FLAT if "flat" in path else GNV_QUAD) for p in (GN_FWD_SUMS, GN_APPLY)), (path, B, HW, C)
            _gn_case(dt, B, HW, C, film, silu, seed=100 + i)
    finally:
        lib().vaw_debug_gn_flat(-1)


# ---- packed dropout -------------------------------------------------------------------------------------------------------------
def _bf16_ulp(ref):
    return torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120))) - 7)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,C", [(1, 8), (33, 8), (513, 8), (4096, 256)])         # M C = 8, 264, 4096 + 8, 1 << 20
def test_packed_dropout_is_vaw_mul_with_the_unpacked_mask(dt, p, M, C):
    """pack -> bits_fwd / bits_bwd against vaw_mul with the unpacked mask: bitwise.  Against float64: the product of the kernel's own
    inputs, x and the act-dtype mask keep / (1 - p), to test_gpu_rows.py's tolerance for one operation in the output dtype (bf16:
    one bf16 ulp; f32: rtol 1e-5), and the ideal x keep / (1 - p) to that plus the rounding of the mask value to the act dtype
    (bf16: 2^-9 relative; f32: inside the rtol).  Sizes: one mask byte, a partial last word (264 = 8 words + 8 bits), more than one
    block with a partial last word, and 2^20 (grid-stride)."""
    td, n = TORCH_DT[dt], M * C
    g = torch.Generator().manual_seed(M + C)
    x, dy = (torch.randn(M, C, generator=g) * 2).to(DEV, td), torch.randn(M, C, generator=g).to(DEV, td)
    torch.manual_seed(11)
    keep = torch.rand(M, C, device=DEV) < (1 - p)
    mask = keep.to(td).mul_(1.0 / (1 - p))                                  # as UNetModel._dropout draws it
    ks = float(torch.ones(1, dtype=td).mul_(1.0 / (1 - p)))                  # as UNetModel._keep_scale makes it
    assert ks == float(mask.max()) or not bool(keep.any())
    words = lib().vaw_dropout_bits_words(n)
    assert words == (n + 31) // 32
    bits = torch.full((words + 4,), 0x5a5a5a5a, device=DEV, dtype=torch.int32)          # canary words behind
    assert lib().vaw_dropout_pack(dt, ptr(mask), ptr(bits), M, C, stream_ptr()) == 0
    assert bool((bits[words:] == 0x5a5a5a5a).all())
    got_bits = np.unpackbits(bits[:words].cpu().numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(got_bits[:n], keep.flatten().cpu().numpy().astype(np.uint8)) and not got_bits[n:].any()
    for src, fn in ((x, lib().vaw_dropout_bits_fwd), (dy, lib().vaw_dropout_bits_bwd)):
        ref = torch.empty_like(src)
        assert lib().vaw_mul(dt, ptr(src), ptr(mask), ptr(ref), n, stream_ptr()) == 0
        out = torch.full((M + 1, C), 7.0, device=DEV, dtype=td)
        assert fn(dt, ptr(src), ptr(bits), ks, ptr(out), n, stream_ptr()) == 0
        assert torch.equal(out[:M], ref) and bool((out[M:] == 7.0).all())
        got = out[:M].double().cpu()
        r64 = src.double().cpu() * mask.double().cpu()
        ideal = src.double().cpu() * keep.double().cpu() / (1 - p)
        if dt == BF16:
            assert bool(((got - r64).abs() <= _bf16_ulp(r64)).all())
            assert bool(((got - ideal).abs() <= _bf16_ulp(ideal) + 2.0 ** -9 * ideal.abs()).all())
        else:
            assert bool(((got - r64).abs() <= 1e-5 * r64.abs()).all())
            assert bool(((got - ideal).abs() <= 1e-5 * ideal.abs()).all())


# ---- engine ---------------------------------------------------------------------------------------------------------------------
def test_trainer_trajectory_tiny_unet_with_activation_checkpointing():
    """test_gpu_unet.py::test_trainer_trajectory_tiny_unet_learned_variance_vs_reference with args.activation_checkpointing=True: the
    Trainer switches the flag on (the model is built with it off) and the run lands on the same fixture within the same 1e-4."""
    exp = load_json("trainer_vb.json")["unet_tiny_learn_sigma"]
    args = base_args(image_size=16, lr=1e-3, learn_sigma=True, cpu_rng=True, activation_checkpointing=True)
    random.seed(42); np.random.seed(42); torch.manual_seed(42)
    model = vaw_amd.UNetModel(16, 3, 32, 6, 1, attention_resolutions=(2,), channel_mult=(1, 2), num_heads=2,
                              use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True,
                              compute_dtype="fp32").to(DEV)
    assert not model.activation_checkpointing
    ema_model = copy.deepcopy(model)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule(args.path_type, 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.LEARNED_RANGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, synth_loader(8, 3, 16, 3, 0), Pbar())
    assert model.activation_checkpointing
    losses = [tr.train_step(s) for s in range(1, 6)]
    assert model._ckpt_fwd
    np.testing.assert_allclose(losses, exp["losses"], rtol=1e-4)
    psum = float(sum(p.double().abs().sum() for p in model.parameters()))
    esum = float(sum(v.double().abs().sum() for v in ema_model.state_dict().values()))
    assert psum == pytest.approx(exp["param_abs_sum"], rel=1e-5)
    assert esum == pytest.approx(exp["ema_abs_sum"], rel=1e-6)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_no_grad_forward_between_forward_and_backward(dtype):
    """A torch.no_grad() forward (other inputs, eval-style) between a checkpointed training forward and its backward leaves the
    pending units, their saved statistics and the gradients untouched."""
    x, t, y, gout = _inputs(2, 16)
    x2, t2, y2, _ = _inputs(2, 16, seed=9)
    ref = _step(_model(dtype, True), x, t, y, gout)
    m = _model(dtype, True)

    def between():
        with torch.no_grad():
            o = m(x2, t2, y=y2)
        assert bool(torch.isfinite(o).all())
    _assert_same(_step(m, x, t, y, gout, between=between), ref, f"interleaved no_grad forward, {dtype}")


@pytest.mark.parametrize("first", [False, True])
def test_flag_switched_between_forward_and_backward_is_refused(first):
    x, t, y, gout = _inputs(2, 16)
    m = _model("fp32", first)
    out = m(x, t, y=y)
    m.set_activation_checkpointing(not first)
    with pytest.raises(vaw_amd.VawError, match="activation_checkpointing"):
        (out * gout).sum().backward()
    m.set_activation_checkpointing(first)          # switched back: the tape is still the forward's
    (out * gout).sum().backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


def test_backward_stage_hooks_with_the_flag_on():
    """The DDP stages with checkpointed units: same order, and every stage's gradients are final when its hook fires (the
    deferred weight gradients of a unit are flushed inside the unit's closure, before the stage closure runs)."""
    x, t, y, gout = _inputs(2, 16)
    for dtype in ("bf16", "fp32"):
        m = _model(dtype, True)
        m.ensure_flat()
        bounds = m.grad_stage_bounds()
        assert set(bounds) == {3, 2, 0}
        snaps = []
        m.grad_ready_hook = lambda st: snaps.append((st, m.flat_grads()[bounds[st][0]:bounds[st][1]].clone()))
        (m(x, t, y=y) * gout).sum().backward()
        m.grad_ready_hook = None
        assert [s for s, _ in snaps] == [3, 2, 0]
        final = m.flat_grads()
        for st, snap in snaps:
            assert torch.equal(snap, final[bounds[st][0]:bounds[st][1]]), (dtype, st)
            assert float(snap.abs().max()) > 0


def test_hip_graph_step_with_the_flag_on_matches_the_eager_step():
    """args.hip_graph with args.activation_checkpointing: the recomputation is a fixed launch sequence, so the step is captured;
    with the weight-gradient deferral off (a captured step never defers) the captured and the eager steps are the same kernels and
    the trajectories are equal bit for bit.  dropout = 0.1 from the device generator: the captured mask bits are replayed."""
    class FixedDraws(vaw_amd.GaussianDiffusion):
        def training_losses(self, model, x_start, features=None, t=None, model_kwargs=None, noise=None):
            return super().training_losses(model, x_start, features, t=self._t, model_kwargs=model_kwargs, noise=self._noise)

    def run(graph, dropout):
        args = base_args(image_size=16, lr=1e-3, grad_clip=0.5, defer_loss_sync=True, hip_graph=graph, activation_checkpointing=True)
        random.seed(42); np.random.seed(42); torch.manual_seed(42)
        model = vaw_amd.UNetModel(16, 3, 32, 3, 1, attention_resolutions=(1, 2), channel_mult=(1, 2), num_heads=2, use_scale_shift_norm=True,
                                  resblock_updown=True, use_new_attention_order=True, dropout=dropout, compute_dtype="bf16").to(DEV)
        perturb_(model, 5)
        model._grouped_wgrad = False
        ema_model = copy.deepcopy(model)
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, eps=1e-8)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = FixedDraws(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                          model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        g = torch.Generator().manual_seed(9)
        diff._t = torch.randint(0, 1000, (8,), generator=g).to(DEV)
        diff._noise = torch.randn(8, 3, 16, 16, generator=g).to(DEV)
        batches = [(torch.randn(8, 3, 16, 16, generator=g), torch.zeros(8, dtype=torch.long)) for _ in range(3)]
        tr = vaw_amd.Trainer(args, torch.device(DEV), model, ema_model, opt, sched, diff, batches, Pbar())
        losses = [float(tr.train_step(s)) for s in range(1, 5)]
        assert model.activation_checkpointing and model._ckpt_fwd
        return losses, model._flat.clone()

    le, pe = run(False, 0.0)
    lg, pg = run(True, 0.0)
    assert all(np.isfinite(le)) and le == lg and torch.equal(pe, pg)
    ld, pd = run(True, 0.1)          # device-RNG dropout inside the captured step: trains, and differs from the run without dropout
    assert all(np.isfinite(ld)) and bool(torch.isfinite(pd).all()) and ld != lg

"""Whole-model gradients of the HIP DiT and UNet on the bf16 and fp8 paths against the float64 oracle, tensor by tensor.

Every case of tests/model_grad_cases.py: the oracle's weights are loaded into the vaw_amd model, one forward and backward run with
the oracle's inputs, and the output, the input gradient and EVERY parameter gradient are held, as whole tensors, to

    ||hip - g64|| / ||g64||  <=  margin * e_ref          (e_ref: the oracle's own bf16-autocast / fake-fp8 distance from float64)

-- the criterion tests/test_model_grad_cases_cpu.py shows to reject a swapped q / k block, a permuted head, two blocks' gradients in
each other's slot, a transposed square gradient, a wrong sign and a dropped K tile, none of which a norm sees.  Each case also
asserts that the branch it is named for ran, that the same wiring errors put into the HIP gradients are rejected, that a second backward after zero_grad_flat has the same bits, and that two backwards
without zeroing give twice the gradient.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

import model_grad_cases as C

pytestmark = pytest.mark.gpu

import vaw_amd

DEV = "cuda"
# two backwards onto one buffer: every element is the first pass's value plus the same value again, summed in f32 in whatever order
# the launch's partial sums arrive -- a few ulp (6e-8) per element; 1e-6 relative L2 leaves 16
ACCUM_TOL = 1e-6


def _build(case, **attrs):
    om = C.build_oracle(case)
    opts = case.hip_opts
    if case.family == "dit":
        hm = vaw_amd.DiT(compute_dtype=case.mode, activation_checkpointing=opts.get("activation_checkpointing", False), **case.kwargs)
    else:
        hm = vaw_amd.UNetModel(compute_dtype=case.mode, use_checkpoint=opts.get("use_checkpoint", False), **case.kwargs)
    hm.load_state_dict(om.state_dict())
    hm = hm.to(DEV).train()
    for k in ("defer_wgrad", "fp8_scaling", "fp8_grad_format"):
        if k in opts:
            setattr(hm, k, opts[k])
    if "grouped_wgrad" in opts:
        hm._grouped_wgrad = opts["grouped_wgrad"]
    for k, v in attrs.items():
        assert hasattr(hm, k)
        setattr(hm, k, v)
    return hm


def _inputs(case):
    x, t, y, gout = (v.to(DEV) for v in C.inputs(case))
    return x.requires_grad_(True), t, y, gout


def _backward(case, hm, inp):
    """One forward and backward -> {OUT, GX, name: gradient} (clones, on the device)."""
    x, t, y, gout = inp
    x.grad = None
    out = hm(x, t, y)[0] if case.family == "dit" else hm(x, t, y=y)
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    res = {C.OUT: out.detach().clone(), C.GX: x.grad.clone()}
    for k, p in hm.named_parameters():
        if p.requires_grad:
            res[k] = None if p.grad is None else p.grad.clone()
    return res


def _hold(case, got, record_property, tag=""):
    g64 = C.reference(case)
    _, e_ref = C.case_yardstick(case)
    fails, worst = C.criterion(case, got, g64, e_ref)
    ratios = sorted(((C.rel_err(got[k], g64[k]) / e_ref[k], k) for k in g64 if got.get(k) is not None), reverse=True)
    print(f"\n{case.id}{tag}: worst rel_err / e_ref = {worst[0]:.3f} at {worst[1]} (rel_err {worst[2]:.5f}, e_ref {worst[3]:.5f}); "
          f"@out {C.rel_err(got[C.OUT], g64[C.OUT]) / e_ref[C.OUT]:.3f}, @gx {C.rel_err(got[C.GX], g64[C.GX]) / e_ref[C.GX]:.3f}; "
          "next: " + ", ".join(f"{r:.3f} {k}" for r, k in ratios[1:5]))
    record_property(f"worst_ratio{tag}", round(worst[0], 4))
    record_property(f"worst_tensor{tag}", worst[1])
    record_property(f"worst_rel_err{tag}", worst[2])
    record_property(f"worst_e_ref{tag}", worst[3])
    assert not fails, [(k, f"rel_err {e:.5f} > bound {b:.5f} (e_ref {e_ref[k]:.5f})") for k, e, b in fails]


def _assert_branch(case, hm, seen):
    """The branch the case is named for was taken, read from what the models expose."""
    opts = case.hip_opts
    if case.family == "unet":
        assert hm._dt == vaw_amd._lib.BF16 and not hm._pend_wgrad          # everything queued was flushed
        assert bool(hm._grouped_wgrad) == opts.get("grouped_wgrad", True)
        assert bool(hm._wgrad_groups) == opts.get("grouped_wgrad", True)     # 1x1 weight gradients went through a WgradGroup (or none did)
        assert hm._ckpt_fwd == hm.activation_checkpointing == opts.get("use_checkpoint", False)
        kw = case.kwargs
        assert hm.input_blocks[3][1].attention.new_order == kw["use_new_attention_order"]
        assert isinstance(hm.input_blocks[2][0], vaw_amd.unet.ResBlock) == kw["resblock_updown"]
        return
    ws, L_ = hm._ws_cur, hm.depth
    assert ws.B == case.batch and ws.fp8 == (case.mode == "fp8") and ws.ckpt == opts.get("activation_checkpointing", False)
    assert hm.defer_wgrad == opts.get("defer_wgrad", True) and ws.defer == hm.defer_wgrad
    spans = sorted((k[0], k[1]) for k in ws.wgrad_groups)
    if not hm.defer_wgrad:
        assert spans == []
    elif ws.ckpt:
        assert spans == [(l, l) for l in range(L_)] and ws.plan.records == 1          # one grouped launch per recomputed block
    elif opts.get("hook"):
        assert L_ >= 4 and spans == [(0, L_ // 2 - 1), (L_ // 2, L_ - 1)]
        # head; the upper half's stages as their grouped launch finishes (in launch order); the early adaLN bucket; the lower half; rest
        assert seen == [L_ + 1] + list(range(L_ // 2 + 1, L_ + 1)) + ["ada_hi"] + list(range(1, L_ // 2 + 1)) + [0], seen
    else:
        assert spans == [(0, L_ - 1)]
    if not opts.get("hook"):
        assert seen == []
    if case.mode == "fp8":
        delayed = hm.fp8_scaling == "delayed"
        assert hm.fp8_grad_format == opts["fp8_grad_format"] and ws.d_fwd == ws.d_bwd == delayed
        assert (case.batch * hm.T) % 128 == 0 and hm.D % 128 == 0 and hm.Dm % 128 == 0
    kw = case.kwargs
    assert (hm.T, hm.D // hm.num_heads, hm.patch_size, hm.No) == ((kw["image_size"] // kw["patch_size"]) ** 2, kw["hidden_size"] // kw["num_heads"],
                                                                  kw["patch_size"], kw["patch_size"] ** 2 * (8 if kw["learn_sigma"] else 4))
    assert (hm._ada_split_block() is None) == (L_ < 4)
    # the attention kernels block 0 ran on, from the launch plan at its own addresses
    L, ops, b, es = vaw_amd._lib, vaw_amd.ops, ws.blk[0], 2
    q, dq = L.ptr(b["qkv"]), L.ptr(b["dqkv"] if "dqkv" in b else ws.dqkv)
    qkv = lambda p: (p, p + es * hm.D, p + 2 * es * hm.D)
    fwd = L.AV_NAMES[ops.attn_plan(L.ATTN_FWD, L.BF16, hm._attn_desc(ws.B), *qkv(q), L.ptr(b["ao"])).variant]
    bwd = L.AV_NAMES[ops.attn_plan(L.ATTN_BWD_COLSUM if ws.defer else L.ATTN_BWD, L.BF16, hm._attn_desc(ws.B), *qkv(q), L.ptr(ws.dao), *qkv(dq)).variant]
    if hm.T == 64:
        assert (fwd, bwd) == ("fwd_t64", "bwd_t64")
    elif hm.T == 256:
        assert fwd in ("fwd_g1", "fwd_g2", "fwd_big") and bwd in ("bwd_g1", "bwd_g2", "bwd_big_nt2", "bwd_big_nt4")     # the MFMA families at head dim 96
    else:
        assert (fwd, bwd) == ("rowwise", "rowwise") and hm.T == 16


def _mutated_hip_gradients_are_rejected(case, got):
    """The CPU test mutates the float64 gradients; here the same wiring errors are put into the HIP model's OWN gradients (its
    rounding included) and the criterion has to reject each one at every tensor it touched."""
    g64 = C.reference(case)
    _, e_ref = C.case_yardstick(case)
    host = {k: v.double().cpu() for k, v in got.items()}
    muts = C.mutations(case, host)
    assert len(muts) >= 8
    for name, label, changed in muts:
        fails, _ = C.criterion(case, C.mutate(host, changed), g64, e_ref, keys=list(changed))
        assert {k for k, _, _ in fails} == set(changed), (name, label, fails)


def _equal_bits(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("case", [c for c in C.CASES if c.id != "dit_fp8_delayed"], ids=lambda c: c.id)
def test_model_gradients_vs_float64_oracle(case, record_property):
    hm = _build(case)
    seen = []
    if case.hip_opts.get("hook"):
        hm.grad_ready_hook = seen.append
    inp = _inputs(case)
    g1 = _backward(case, hm, inp)
    _assert_branch(case, hm, seen)
    _hold(case, g1, record_property)
    _mutated_hip_gradients_are_rejected(case, g1)
    # the model's own zeroing call, then the same backward: the same bits
    hm.zero_grad_flat()
    g2 = _backward(case, hm, inp)
    assert _equal_bits(g1, g2) == []
    # no zeroing: the gradients add (the output and the input gradient do not)
    g3 = _backward(case, hm, inp)
    assert torch.equal(g3[C.OUT], g1[C.OUT]) and torch.equal(g3[C.GX], g1[C.GX])
    worst = max((C.rel_err(g3[k], 2 * g1[k].double().cpu()), k) for k in g1 if k not in (C.OUT, C.GX))
    assert worst[0] <= ACCUM_TOL, worst


def test_model_gradients_fp8_delayed_scaling(record_property):
    """The default fp8 recipe: two passes on one batch with zero_grad_flat between them; the SECOND, whose scales come from the
    first, is held to the criterion -- with the fused fp8 epilogues / row passes and with the separate quantisers, which must also
    agree bit for bit."""
    case = C.BY_ID["dit_fp8_delayed"]
    res = {}
    for fuse in (True, False):
        hm = _build(case, fp8_fuse_epilogue=fuse, fp8_fuse_rows=fuse)
        inp = _inputs(case)
        _backward(case, hm, inp)
        ws = hm._ws_cur
        assert ws.fp8 and not ws.d_fwd and not ws.d_bwd                      # first pass: scales taken just in time
        hm.zero_grad_flat()
        res[fuse] = _backward(case, hm, inp)
        _assert_branch(case, hm, [])
        _hold(case, res[fuse], record_property, tag="_fused" if fuse else "_pair")
    _mutated_hip_gradients_are_rejected(case, res[True])
    assert _equal_bits(res[True], res[False]) == []

"""Per-tensor float64 parity of whole-model gradients on the bf16 and fp8 paths: the case table, the references and the criterion.

CPU-importable (oracle and torch only).  tests/test_model_grad_cases_cpu.py shows on the CPU that the criterion tells rounding from a
wiring error at every case; tests/test_gpu_model_grads.py applies it to the HIP models.

What is compared: the model output ("@out"), the input gradient ("@gx") and EVERY parameter gradient, whole tensors, by

    rel_err(got, g64) = ||got - g64|| / ||g64||          (float64, g64 = the oracle run in float64)

against a yardstick measured on the oracle itself:

    e_ref[k] = rel_err(g_autocast[k], g64[k])              (the same oracle under torch.autocast("cpu", bfloat16): how far CORRECT
                                                            bf16 arithmetic lies from float64 at that tensor)
    criterion:  rel_err(hip[k], g64[k]) <= margin_k * e_ref[k],   margin_k = MARGIN unless the case names a class of tensors

The fp8 cases use the same oracle with the blocks' four Linear layers fake-quantised (yardstick_fp8).  The cap keeps a margin from
growing into the range of a wiring error: margin_k * e_ref[k] must stay below half of the smallest error any mutation that touches
k produces.  MUTATIONS are the wiring errors a norm comparison cannot see.
"""
import contextlib
import functools
import re
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from oracle import dit as odit
from oracle import unet as ounet

MARGIN = 2.0          # the HIP path rounds where autocast does not (bf16 activations between kernels, bf16 dy of the deferred products)
#                       and keeps f32 where autocast rounds (residual stream, row statistics): a factor of 2 covers the former
CAP_FRACTION = 0.5    # margin_k * e_ref[k] < CAP_FRACTION * (smallest mutation error at k)
MIN_RMS_FRACTION = 1e-4      # no tensor is exempt: every gradient's rms is above this fraction of the model's overall gradient rms
OUT, GX = "@out", "@gx"


# ------------------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    family: str                  # "dit" | "unet"
    kw: tuple                    # oracle / HIP model constructor arguments (sorted items of a dict)
    batch: int
    mode: str = "bf16"           # "bf16" | "fp8"
    hip: tuple = ()              # how the HIP model is set up (sorted items): read by tests/test_gpu_model_grads.py
    std: float = 0.05            # perturb_ (adaLN-Zero / zero-initialised convolutions would leave most gradients exactly 0)
    seed: int = 0
    # per-class margins above MARGIN: (regex on the tensor name, margin, the extra rounding point in the code that explains it)
    margins: tuple = field(default=())

    @property
    def kwargs(self):
        return dict(self.kw)

    @property
    def hip_opts(self):
        return dict(self.hip)


def _dit(id, hidden, depth, heads, px, patch, batch, learn_sigma=False, mode="bf16", seed=0, margins=(), **hip):
    kw = dict(image_size=px, patch_size=patch, in_channels=4, hidden_size=hidden, depth=depth, num_heads=heads, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=learn_sigma)
    return Case(id, "dit", tuple(sorted(kw.items())), batch, mode, tuple(sorted(hip.items())), 0.05, seed, tuple(margins))


def _unet(id, new, out, seed=0, margins=(), **hip):
    kw = dict(image_size=16, in_channels=3, model_channels=64, out_channels=out, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 2), num_heads=2, num_classes=10, use_scale_shift_norm=new, resblock_updown=new, use_new_attention_order=new)
    return Case(id, "unet", tuple(sorted(kw.items())), 4, "bf16", tuple(sorted(hip.items())), 0.03, seed, tuple(margins))


CASES = [
    # one grouped launch for all blocks, head with 2 C outputs
    _dit("dit_defer", 128, 4, 2, 8, 2, 16, learn_sigma=True),
    # two grouped launches, early adaLN bucket (depth >= 4)
    _dit("dit_defer_hook", 128, 4, 2, 8, 2, 16, learn_sigma=True, hook=True),
    # per-layer weight gradients
    _dit("dit_perlayer", 128, 4, 2, 8, 2, 16, learn_sigma=True, defer_wgrad=False),
    # recompute record
    _dit("dit_ckpt", 128, 4, 2, 8, 2, 16, learn_sigma=True, activation_checkpointing=True),
    # head dim 32, T = 64 attention
    _dit("dit_hd32_t64", 128, 2, 4, 16, 2, 4),
    # head dim 96, T = 256, shallow (no adaLN split)
    _dit("dit_hd96_t256", 192, 2, 2, 32, 2, 2),
    # patch 4 embed / unpatchify
    _dit("dit_p4", 128, 2, 2, 16, 4, 16),
    # fp8 blocks (D, Dm % 128; M = 256), scales measured just in time, both gradient formats
    _dit("dit_fp8_jit_e5m2", 128, 2, 2, 8, 2, 16, mode="fp8", fp8_scaling="jit", fp8_grad_format="e5m2"),
    _dit("dit_fp8_jit_e4m3", 128, 2, 2, 8, 2, 16, mode="fp8", fp8_scaling="jit", fp8_grad_format="e4m3"),
    # default recipe: the SECOND pass on one batch is checked, its scales come from the first
    _dit("dit_fp8_delayed", 128, 2, 2, 8, 2, 16, mode="fp8", fp8_scaling="delayed", fp8_grad_format="e5m2"),
    # scale-shift norm, resblock up/down, new attention order; 1x1 weight gradients grouped per stage
    _unet("unet_new", True, 3),
    # none of the three: conv up / stride-2 down, legacy attention order, 6 outputs
    _unet("unet_legacy", False, 6),
    _unet("unet_perlayer", True, 3, grouped_wgrad=False),
    _unet("unet_ckpt", True, 3, use_checkpoint=True),
]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


def perturb_(model, seed, std):
    """tests/conftest.py::perturb_ (this module imports nothing from the test tree)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.add_((torch.randn(p.shape, generator=g) * std).to(p.device))


def build_oracle(case):
    """The oracle model of a case in f32, train mode, moved off its zero initialisation."""
    torch.manual_seed(100 + case.seed)
    om = (odit.DiT if case.family == "dit" else ounet.UNetModel)(**case.kwargs)
    perturb_(om, 200 + case.seed, case.std)
    return om.train()


def inputs(case):
    """(x, t, y, gout) from a seeded CPU generator.  The UNet input is 4 x randn, the amplitude of the synthetic latents of the
    trainer tests: the bf16 yardstick of this UNet falls with the amplitude of its input (worst tensor over three seeds: 4.7-5.4 %
    for images in [-1, 1], 3.5-4.8 % at unit variance, 3.3-3.9 % at 2, 2.6-2.8 % at 4), and twice the yardstick has to stay under
    half of the mildest mutation (6.25 %): test_model_grad_cases_cpu.py asserts that it does."""
    kw, B = case.kwargs, case.batch
    g = torch.Generator().manual_seed(300 + case.seed)
    px = kw["image_size"]
    if case.family == "dit":
        x = torch.randn(B, 4, px, px, generator=g)
        co = 8 if kw["learn_sigma"] else 4
    else:
        x = torch.randn(B, 3, px, px, generator=g) * 4
        co = kw["out_channels"]
    t = torch.rand(B, generator=g) * 999.0
    y = torch.randint(0, 10, (B,), generator=g)
    gout = torch.randn(B, co, px, px, generator=g)
    return x, t, y, gout


# ------------------------------------------------------------------------------------------------------------------------------
# oracle runs
# ------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _float64_oracle(om):
    """Lift the places where the oracle casts to f32 INSIDE the model, for the duration of a float64 run, without touching oracle/:
    the timestep embedding (built in f32, fed to the embedding MLP), GroupNorm32.forward (x.float()) and the f32 softmax of the UNet
    attention.  reference_matches_f32() shows the patch changes nothing else."""
    mlp = om.t_embedder.mlp if hasattr(om, "t_embedder") else om.time_embed
    hook = mlp.register_forward_pre_hook(lambda mod, a: (a[0].double(),))
    gn_forward, attend = ounet.GroupNorm32.forward, ounet._attend

    def attend64(q, k, v, ch):
        s = 1 / (float(ch) ** 0.25)
        w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
        return torch.einsum("bts,bcs->bct", w, v)

    ounet.GroupNorm32.forward = lambda self, x: nn.GroupNorm.forward(self, x)
    ounet._attend = attend64
    try:
        yield
    finally:
        hook.remove()
        ounet.GroupNorm32.forward, ounet._attend = gn_forward, attend


def _call(family, om, x, t, y):
    if family == "dit":
        return om(x, t, y)[0]
    return om(x, t, y=y) if y is not None else om(x, t)


def run_oracle(family, om, x, t, y, gout, mode):
    """One forward and backward of `om` (f32 weights, left unchanged) -> {OUT, GX, <parameter name>: gradient}, all float64 on the CPU.
    mode: "f64" (the reference), "f32" (the oracle as it stands), "bf16" (torch.autocast("cpu", bfloat16), the reference's own bf16
    mode), "fp8:e5m2" / "fp8:e4m3" (autocast with the blocks' Linear layers fake-quantised, DiT only)."""
    import copy
    m = copy.deepcopy(om)
    m.zero_grad(set_to_none=True)
    ctx = contextlib.nullcontext()
    if mode == "f64":
        m = m.double()
        x, gout = x.double(), gout.double()
        ctx = _float64_oracle(m)
    elif mode.startswith("fp8"):
        assert family == "dit"
        fmt = {"e5m2": torch.float8_e5m2, "e4m3": torch.float8_e4m3fn}[mode.split(":")[1]]
        for blk in m.blocks:
            for holder, name in ((blk.attn, "qkv"), (blk.attn, "proj"), (blk.mlp, "fc1"), (blk.mlp, "fc2")):
                setattr(holder, name, FakeQuantLinear(getattr(holder, name), fmt))
    xr = x.clone().requires_grad_(True)
    with ctx:
        if mode in ("f64", "f32"):
            out = _call(family, m, xr, t, y)
        else:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = _call(family, m, xr, t, y)
        (out.to(gout.dtype) * gout).sum().backward()
    res = {OUT: out.detach().double(), GX: xr.grad.double()}
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, k
            res[k.replace(".lin.", ".")] = p.grad.double()
    return res


class _FakeQuantFn(torch.autograd.Function):
    """y = q(x) q(W)^T + b with x, W rounded through e4m3 and, in backward, dy through `fmt`; per-tensor scale amax / finfo.max,
    products in f32.  What fp8 means, restated -- not a model of the HIP recipe (no margin, no delayed scales)."""

    @staticmethod
    def q(v, fmt):
        v = v.float()
        amax = float(v.abs().max())
        if amax == 0.0:
            return v
        s = amax / torch.finfo(fmt).max
        return (v / s).to(fmt).float() * s

    @staticmethod
    def forward(ctx, x, w, b, fmt):
        xq, wq = _FakeQuantFn.q(x, torch.float8_e4m3fn), _FakeQuantFn.q(w, torch.float8_e4m3fn)
        ctx.save_for_backward(xq, wq)
        ctx.fmt, ctx.xdt = fmt, x.dtype
        return (xq @ wq.t() + b.float()).to(torch.bfloat16)

    @staticmethod
    def backward(ctx, dy):
        xq, wq = ctx.saved_tensors
        dyq = _FakeQuantFn.q(dy, ctx.fmt)
        dx = (dyq @ wq).to(ctx.xdt)
        dw = dyq.reshape(-1, dyq.shape[-1]).t() @ xq.reshape(-1, xq.shape[-1])
        return dx, dw, dy.float().reshape(-1, dy.shape[-1]).sum(0), None


class FakeQuantLinear(nn.Module):
    def __init__(self, lin, fmt):
        super().__init__()
        self.lin, self.fmt = lin, fmt

    def forward(self, x):
        return _FakeQuantFn.apply(x, self.lin.weight, self.lin.bias, self.fmt)


@functools.lru_cache(maxsize=None)
def _runs(case_id, mode):
    case = BY_ID[case_id]
    return run_oracle(case.family, build_oracle(case), *inputs(case), mode)


def reference(case):
    """The oracle's output, input gradient and every parameter gradient in float64.  Computed once per case; do not modify."""
    return _runs(case.id, "f64")


def reference_f32(case):
    return _runs(case.id, "f32")


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).norm() / ref.norm())


def errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in ref}


def yardstick(case):
    """-> (gradients of the bf16-autocast oracle, e_ref): the distance of correct bf16 arithmetic from float64, per tensor."""
    g = _runs(case.id, "bf16")
    return g, errors(g, reference(case))


def yardstick_fp8(case, grad_fmt):
    g = _runs(case.id, f"fp8:{grad_fmt}")
    return g, errors(g, reference(case))


def case_yardstick(case):
    """The yardstick the case's mode is held to."""
    return yardstick(case) if case.mode == "bf16" else yardstick_fp8(case, case.hip_opts["fp8_grad_format"])


# ------------------------------------------------------------------------------------------------------------------------------
# criterion
# ------------------------------------------------------------------------------------------------------------------------------
def margin_for(case, key):
    for pat, m, _reason in (case.margins if case is not None else ()):
        if re.search(pat, key):
            return float(m)
    return MARGIN


def bounds(case, e_ref):
    return {k: margin_for(case, k) * e for k, e in e_ref.items()}


def criterion(case, got, g64, e_ref, keys=None):
    """-> (failures, worst): failures = [(key, rel_err, bound)] of the tensors beyond margin_k * e_ref[k] (a missing tensor fails);
    worst = (rel_err / e_ref, key, rel_err, e_ref) over the tensors looked at.  `case` may be None (MARGIN everywhere)."""
    fails, worst = [], (0.0, None, 0.0, 0.0)
    for k in (g64 if keys is None else keys):
        if k not in got or got[k] is None:
            fails.append((k, float("inf"), margin_for(case, k) * e_ref[k]))
            continue
        e = rel_err(got[k], g64[k])
        if not e <= margin_for(case, k) * e_ref[k]:
            fails.append((k, e, margin_for(case, k) * e_ref[k]))
        if e / e_ref[k] > worst[0]:
            worst = (e / e_ref[k], k, e, e_ref[k])
    return fails, worst


def oracle_yardstick(family, om, x, t, y, gout):
    """-> (g64, e_ref) of any oracle model and inputs (the model-level tests that bring their own sizes)."""
    g64 = run_oracle(family, om, x, t, y, gout, "f64")
    return g64, errors(run_oracle(family, om, x, t, y, gout, "bf16"), g64)


def hold_whole_tensors(got, g64, e_ref):
    """The criterion at MARGIN on the output, the input gradient and every parameter gradient whose float64 rms is above
    MIN_RMS_FRACTION of the overall one (at sizes this module did not choose a gradient can be exactly zero: a convolution bias
    in front of a GroupNorm with one channel per group).  -> (worst, number of tensors held); raises on a tensor beyond its bound."""
    frac = rms_fractions(g64)
    keys = [k for k in g64 if frac.get(k, 1.0) > MIN_RMS_FRACTION]
    fails, worst = criterion(None, got, g64, e_ref, keys)
    assert not fails, [(k, f"rel_err {e:.5f} > {MARGIN} x e_ref {e_ref[k]:.5f}") for k, e, _ in fails]
    return worst, len(keys)


def rms_fractions(g64):
    """rms of every parameter gradient over the rms of all parameter gradients together."""
    ks = [k for k in g64 if k not in (OUT, GX)]
    total = (sum(float(g64[k].pow(2).sum()) for k in ks) / sum(g64[k].numel() for k in ks)) ** 0.5
    return {k: float(g64[k].pow(2).mean().sqrt()) / total for k in ks}


# ------------------------------------------------------------------------------------------------------------------------------
# mutations: structurally wrong gradients of unchanged (or nearly unchanged) norm
# ------------------------------------------------------------------------------------------------------------------------------
def _swap_rows(v, a, b, n):
    v = v.clone()
    v[a:a + n], v[b:b + n] = v[b:b + n].clone(), v[a:a + n].clone()
    return v


def _m_sign(case, g):
    """the sign of one tensor (a subtraction the wrong way round, a beta of -1)"""
    k = "blocks.1.mlp.fc1.weight" if case.family == "dit" else "middle_block.0.in_layers.2.weight"
    yield k, {k: -g[k]}


def _m_qk_swap(case, g):
    """the q and k row blocks of one qkv weight exchanged (DiT: [q | k | v] rows of the packed Linear)"""
    if case.family == "dit":
        k, D = "blocks.0.attn.qkv.weight", case.kwargs["hidden_size"]
        yield k, {k: _swap_rows(g[k], 0, D, D)}


def _m_head_swap(case, g):
    """two heads' row blocks exchanged within q (a head index applied to the wrong stride)"""
    if case.family == "dit":
        kw = case.kwargs
        k, hd = f"blocks.{kw['depth'] - 1}.attn.qkv.weight", kw["hidden_size"] // kw["num_heads"]
        yield k, {k: _swap_rows(g[k], 0, hd, hd)}


def _m_block_swap(case, g):
    """block i <-> block j for one same-shaped tensor (problem i of a grouped launch writing into problem j's slot)"""
    a, b = (("blocks.0.mlp.fc2.weight", "blocks.1.mlp.fc2.weight") if case.family == "dit"
            else ("middle_block.0.in_layers.2.weight", "middle_block.2.in_layers.2.weight"))
    assert g[a].shape == g[b].shape
    yield f"{a} <-> {b}", {a: g[b], b: g[a]}


def _m_transpose(case, g):
    """one square weight transposed (dy^T x computed as x^T dy)"""
    k = "blocks.0.attn.proj.weight" if case.family == "dit" else "middle_block.1.proj_out.weight"
    assert g[k].shape[0] == g[k].shape[1]
    yield k, {k: g[k].transpose(0, 1).contiguous()}


def _m_adaln_chunk(case, g):
    """one adaLN chunk (D rows of the 6 D: shift1 scale1 gate1 shift2 scale2 gate2) exchanged with its neighbour"""
    if case.family == "dit":
        D = case.kwargs["hidden_size"]
        k = "blocks.1.adaLN_modulation.1.weight"
        # shift <-> scale (both small next to the gate rows: 0.12 of the tensor) and scale <-> gate (0.9); fp8 cases take the
        # second pair only, for the reason given at scale_7_8 (the tensor's fp8 yardstick is 5.4 %)
        for c in ((0, 3, 1, 4) if case.mode == "bf16" else (1, 4)):
            yield f"{k} chunk {c} <-> {c + 1}", {k: _swap_rows(g[k], c * D, (c + 1) * D, D)}


def _m_scale_7_8(case, g):
    """one tensor scaled by 7/8: a grouped launch that drops one K tile out of eight.  bf16 cases: applied to EVERY tensor in turn
    (the error is 0.125 whatever the tensor), so the cap bounds every tensor of the case: margin_k * e_ref[k] < 0.0625.
    fp8 cases: applied to the head's weight only.  The fp8 yardstick of the blocks' weight gradients is 4-9 % (e4m3 carries 3
    mantissa bits, e5m2 two), so an error of 12.5 % lies within 2 x of CORRECT fp8 rounding and no whole-tensor measure separates
    the two; the fp8 cases are held to the mutations that move a tensor by 25 % or more."""
    for k in (g if case.mode == "bf16" else ["final_layer.linear.weight"]):
        yield k, {k: g[k] * 0.875}


def _m_bias_zero(case, g):
    """one bias gradient zeroed (a fold that never ran, a producer that skipped its column sums)"""
    k = "blocks.0.attn.qkv.bias" if case.family == "dit" else "input_blocks.3.1.qkv.bias"
    yield k, {k: torch.zeros_like(g[k])}


def _m_unet_qkv_order(case, g):
    """UNet: the legacy ([head][q k v][ch]) and the new ([q k v][head][ch]) row order of a qkv weight taken for each other"""
    if case.family == "unet":
        kw = case.kwargs
        k, H = "middle_block.1.qkv.weight", kw["num_heads"]
        v = g[k]
        ch = v.shape[0] // (3 * H)
        yield k, {k: v.reshape(3, H, ch, *v.shape[1:]).transpose(0, 1).reshape(v.shape).contiguous()}


SKIP_OUT_PAIRS = ("input_blocks.3.0.skip_connection.bias", "input_blocks.3.0.out_layers.3.bias")


def _m_unet_skip_out(case, g):
    """UNet: the gradient of a ResBlock's skip connection and of its out_layers.3 exchanged where their shapes agree.  In this
    model family they agree at the biases only (the skip connection is a 1 x 1 convolution, out_layers.3 a 3 x 3 one), and those
    two gradients are the SAME tensor -- both convolutions add onto the block's output, so each bias gradient is the pixel sum of
    the block's output gradient.  Exchanging them is therefore no error and yields no mutation; the CPU test asserts the equality
    (SKIP_OUT_PAIRS) so that this entry is known to be empty for a reason."""
    return
    yield


def _m_unet_doubled(case, g):
    """UNet: one tensor doubled (an accumulation run twice: a deferred weight gradient flushed and also run per layer)"""
    if case.family == "unet":
        k = "output_blocks.0.1.qkv.weight"
        yield k, {k: 2 * g[k]}


MUTATIONS = {
    "sign": _m_sign, "qk_swap": _m_qk_swap, "head_swap": _m_head_swap, "block_swap": _m_block_swap, "transpose": _m_transpose,
    "adaln_chunk": _m_adaln_chunk, "scale_7_8": _m_scale_7_8, "bias_zero": _m_bias_zero, "unet_qkv_order": _m_unet_qkv_order,
    "unet_skip_out": _m_unet_skip_out, "unet_doubled": _m_unet_doubled,
}


def mutations(case, g64):
    """-> [(mutation name, what it touched, {key: wrong tensor})] for every mutation that applies to the case."""
    return [(name, label, changed) for name, fn in MUTATIONS.items() for label, changed in fn(case, g64)]


def mutate(g64, changed):
    """The float64 gradient dict with the mutation's tensors put in (the rest shared, not copied)."""
    return {**g64, **changed}


def smallest_mutation_error(case, g64):
    """-> {key: (smallest rel_err over the mutations that touch key, that mutation)}"""
    small = {}
    for name, label, changed in mutations(case, g64):
        for k, v in changed.items():
            e = rel_err(v, g64[k])
            if k not in small or e < small[k][0]:
                small[k] = (e, f"{name}: {label}")
    return small

"""The fused steps of the linear multistep samplers on the GPU (vaw_dpm_input, vaw_dpm_step): the kernels bitwise the tensor
composition they replace (1 / 2 / 3 nodes, noise, guidance, every prediction type, clamping, in place and out of place, the
final row), dpm_sample with `fused=True` bitwise `fused=False` from the same seed (tiny DiT, tiny UNet, the three solvers,
guidance always / in an interval / off), no host synchronisation once the table is cached, and Sampler's captured graph."""
import itertools

import pytest
import torch

from conftest import perturb_
from sampler_cases import sampler_args

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops, samplers

DEV = "cuda"
SHAPES = [(2, 3, 8, 8), (1, 1, 5, 7), (3, 4, 32, 32)]          # 192 a row; 35: odd row, scalar path; 4096: four blocks a row
SHAPE_IDS = ["2x3x8x8", "1x1x5x7", "3x4x32x32"]
LAYOUTS = ["dense", "slice", "shifted"]
SCALE = 2.5
STEPS = 6


def differ(got, ref):
    return f"{int((got != ref).sum())} of {ref.numel()} elements differ, max |diff| {float((got.double() - ref.double()).abs().max()):.3e}"


def model_output(shape, layout, seed):
    """A stacked [2N, ...] float32 network output for x of `shape`: dense | slice (the [:, :C] part of a [2N, 2C, H, W]
    learn_sigma output: rows 2n apart) | shifted (base one float past a 16-byte boundary)."""
    N, C = shape[:2]
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randn((2 * N, *shape[1:]), generator=g) * 0.7).to(DEV)
    if layout == "slice":
        out = torch.randn((2 * N, 2 * C, *shape[2:]), generator=g).to(DEV)[:, :C]
        assert not out.is_contiguous() and out.stride(0) == 2 * vals[0].numel()
    elif layout == "shifted":
        out = torch.empty(vals.numel() + 1, device=DEV)[1:].view(vals.shape)
        assert out.data_ptr() % 16 == 4
    else:
        out = torch.empty_like(vals)
    out.copy_(vals)
    return out


class Table:
    """The table of dpmpp2m_sde (eta = 1: a, b0, b1 and c of a real grid, and the denoiser's float32 scalars), with weights put
    where that solver has none (b2 everywhere, b1 on the first row), so that every row can be run with 1, 2 or 3 nodes."""
    _made = {}

    @classmethod
    def get(cls, pred_type, batch):
        if (pred_type, batch) not in cls._made:
            net = vaw_amd.EDMDenoiser(torch.nn.Identity(), 8, 3, pred_type=pred_type).to(DEV)
            lo, hi = samplers._edm_sigma_range(net, "edm", None, None, 1e-3)
            tab = samplers._dpm_tables(net, torch.device(DEV), batch, STEPS, lo, hi, 7, "dpmpp2m_sde", None, "edm", 1e-3, 1.0, 1.003)
            coef = tab.coef.clone()
            assert coef.shape == (STEPS, ops.DPM_COLS) and bool((coef[:-1, 4] > 0).all()) and bool((coef[1:-1, 2] < 0).all())
            coef[:, 3] = torch.linspace(0.21, -0.37, STEPS, dtype=torch.float64, device=DEV)
            coef[0, 2], coef[-1, 2], coef[-1, 4] = -0.4375, -0.3, 0.11
            cls._made[pred_type, batch] = coef.contiguous()
        return cls._made[pred_type, batch]


def composed_step(pred_type, clip, row, x, o, d1, d2, noise):
    """(denoised image, x', next network input) as the tensor operations of EDMDenoiser.forward and dpm_sample's composition."""
    sigma = row[5].to(torch.float32).reshape(1, 1, 1, 1)
    c_in = 1 / (sigma ** 2 + 1).sqrt()
    x32 = x.to(torch.float32)
    den = {"EPSILON": lambda: x32 - sigma * o, "START_X": lambda: o, "VELOCITY": lambda: c_in ** 2 * x32 - sigma * c_in * o}[pred_type]()
    if clip:
        den = den.clamp(-1, 1)
    acc = row[0] * x + row[1] * den.to(torch.float64)
    if d1 is not None:
        acc = acc + row[2] * d1.to(torch.float64)
    if d2 is not None:
        acc = acc + row[3] * d2.to(torch.float64)
    if noise is not None:
        acc = acc + row[4] * noise
    return den, acc, row[9].to(torch.float32) * acc.to(torch.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_dpm_input_is_bitwise_the_tensor_composition(shape):
    N = shape[0]
    coef = Table.get("EPSILON", N)
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 80).to(DEV)
    for row, stacked in itertools.product((0, 3), (True, False)):
        ref = coef[row, 6].to(torch.float32) * x.to(torch.float32)
        buf = torch.full((2 * N if stacked else N, *shape[1:]), 7.0, device=DEV)
        ops.dpm_input(x, coef, row, buf[:N], buf[N:] if stacked else None)
        assert torch.equal(buf[:N], ref), (row, differ(buf[:N], ref))
        assert not stacked or torch.equal(buf[N:], ref)
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view(shape)          # scalar path on a misaligned destination
    ops.dpm_input(x, coef, 3, shifted)
    assert torch.equal(shifted, coef[3, 6].to(torch.float32) * x.to(torch.float32))
    with pytest.raises(vaw_amd.VawError, match=f"row {STEPS} outside"):
        ops.dpm_input(x, coef, STEPS, shifted)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_dpm_step_is_bitwise_the_tensor_composition(shape, layout):
    N = shape[0]
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 3).to(DEV)
    nz = torch.randn(shape, generator=g, dtype=torch.float64).to(DEV)
    d1 = torch.randn(shape, generator=g).to(DEV)
    d2 = torch.randn(shape, generator=g).to(DEV)
    out = model_output(shape, layout, 31 + len(layout))
    for pred_type, clip, guided, nodes, noise, row in itertools.product(ops.EDM_PRED, (False, True), (True, False), (1, 2, 3),
                                                                        (True, False), (0, 3)):
        coef = Table.get(pred_type, N)
        what = (pred_type, clip, guided, nodes, noise, row)
        cond, uncond = out[:N], (out[N:] if guided else None)
        o = uncond + SCALE * (cond - uncond) if guided else cond
        h1, h2, z = (d1 if nodes >= 2 else None), (d2 if nodes >= 3 else None), (nz if noise else None)
        den, ref, ref_in = composed_step(pred_type, clip, coef[row], x, o, h1, h2, z)
        assert bool(torch.isfinite(ref).all()) and (not clip or pred_type != "EPSILON" or bool((den.abs() == 1).any()))
        for alias in (False, True):
            x_in = x.clone()
            x_out = x_in if alias else torch.full_like(x, 7.0)
            d0 = torch.full(shape, 7.0, device=DEV)
            buf = torch.full((2 * N, *shape[1:]), 7.0, device=DEV)
            got = ops.dpm_step(pred_type, clip, cond, uncond, SCALE, x_in, h1, h2, z, coef, row, x_out=x_out, d0_out=d0, model_in=buf[:N],
                               model_in_dup=buf[N:] if guided else None)
            assert got is x_out and got.dtype == torch.float64 and torch.equal(got, ref), (what, alias, "x", differ(got, ref))
            assert torch.equal(d0, den), (what, alias, "denoised", differ(d0, den))
            assert torch.equal(buf[:N], ref_in), (what, alias, "next input", differ(buf[:N], ref_in))
            assert torch.equal(buf[N:], ref_in) if guided else bool((buf[N:] == 7.0).all()), (what, alias, "second half")
            assert alias or torch.equal(x_in, x)
    # the final row: a = 0, b0 = 1, x' is the denoised image and no network input is written
    for pred_type, guided in itertools.product(ops.EDM_PRED, (True, False)):
        coef = Table.get(pred_type, N).clone()
        coef[-1, :5] = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
        cond, uncond = out[:N], (out[N:] if guided else None)
        o = uncond + SCALE * (cond - uncond) if guided else cond
        den, ref, _ = composed_step(pred_type, False, coef[-1], x, o, None, None, None)
        x_in, d0 = x.clone(), torch.empty(shape, device=DEV)
        got = ops.dpm_step(pred_type, False, cond, uncond, SCALE, x_in, None, None, None, coef, STEPS - 1, x_out=x_in, d0_out=d0)
        assert torch.equal(got, den.to(torch.float64)) and torch.equal(got, ref) and torch.equal(d0, den), (pred_type, guided, differ(got, ref))
    with pytest.raises(vaw_amd.VawError, match="d2"):
        ops.dpm_step("EPSILON", False, out[:N], None, 1.0, x, None, d2, None, coef, 0, x_out=torch.empty_like(x), d0_out=torch.empty_like(d1))


# ---- loops -----------------------------------------------------------------------------------------------------------------
def tiny_dit(learn_sigma):
    torch.manual_seed(3)
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=3, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.1, num_classes=10,
                    learn_sigma=learn_sigma, compute_dtype="fp32")
    perturb_(m, 17)
    return m.to(DEV).eval()


def tiny_unet(learn_sigma):
    torch.manual_seed(42)
    m = vaw_amd.UNetModel(16, 3, 32, 6 if learn_sigma else 3, 1, attention_resolutions=(2,), channel_mult=(1, 2), num_heads=2, num_classes=10,
                          drop_label_prob=0.1, use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True,
                          compute_dtype="fp32")
    perturb_(m, 23)
    return m.to(DEV).eval()


MODELS = {}


def model_for(name, learn_sigma):
    if (name, learn_sigma) not in MODELS:
        MODELS[name, learn_sigma] = (tiny_dit if name == "dit" else tiny_unet)(learn_sigma)
    return MODELS[name, learn_sigma], (8 if name == "dit" else 16)


GUIDANCE = {"always": (SCALE, (-1.0, -1.0)), "interval": (1.8, (150.0, 700.0)), "off": (1.0, (-1.0, -1.0))}
SOLVERS = {"dpmpp2m": dict(solver="dpmpp2m", clip_denoised=True), "dpmpp2m_sde": dict(solver="dpmpp2m_sde", eta=0.8, s_noise=1.003),
           "expab": dict(solver="expab")}


@pytest.mark.parametrize("guidance", list(GUIDANCE))
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("name", ["dit", "unet"])
def test_dpm_sample_fused_is_bitwise_the_composition(name, solver, guidance):
    model, size = model_for(name, True)
    scale, interval = GUIDANCE[guidance]
    calls = []
    cfg = vaw_amd.IntervalCFG(model, 10, scale, interval, True)
    model.register_forward_pre_hook(lambda m, a: calls.append(a[0].shape[0]))
    net = vaw_amd.EDMDenoiser(cfg, size, 3, pred_type="EPSILON" if name == "dit" else "VELOCITY", label_dim=10).to(DEV)
    y = torch.tensor([1, 5, 9], device=DEV)
    res = []
    try:
        for fused in (False, True):
            torch.manual_seed(11)
            x = vaw_amd.dpm_sample(net, torch.randn(3, 3, size, size, device=DEV), class_labels=y, num_steps=5, fused=fused, **SOLVERS[solver])
            res.append((x, torch.randn(4, device=DEV)))
    finally:
        model._forward_pre_hooks.clear()
    (ref, ref_next), (got, got_next) = res
    assert got.dtype == ref.dtype == torch.float64 and got.shape == ref.shape and bool(torch.isfinite(ref).all())
    assert torch.equal(got, ref), differ(got, ref)
    assert torch.equal(got_next, ref_next), "the generator was left at another offset"
    assert calls[:5] == calls[5:] and len(calls) == 10          # one evaluation per step, guided at the same steps
    stacked = sum(b == 6 for b in calls[:5])
    assert stacked == {"always": 5, "off": 0}.get(guidance, stacked) and (guidance != "interval" or 0 < stacked < 5)


def test_fused_true_refuses_a_denoiser_without_the_chain():
    class Plain:
        sigma_min, sigma_max = 0.002, 80.0
        round_sigma = staticmethod(torch.as_tensor)

        def __call__(self, x, sigma, class_labels=None):
            return 0.2 * x

    z = torch.randn(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.dpm_sample(Plain(), z, num_steps=4, fused=True)
    assert torch.equal(vaw_amd.dpm_sample(Plain(), z, num_steps=4), vaw_amd.dpm_sample(Plain(), z, num_steps=4, fused=False))
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.dpm_sample(vaw_amd.EDMDenoiser(torch.nn.Identity(), 8, 3, pred_type="SCORE").to(DEV), z, num_steps=4, fused=True)


# ---- no host synchronisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dpmpp2m_sde", "expab"])
def test_second_call_does_not_synchronise_with_the_host(solver):
    y = torch.tensor([1, 5, 9], device=DEV)
    model, size = model_for("dit", True)
    net = vaw_amd.EDMDenoiser(vaw_amd.IntervalCFG(model, 10, 1.8, (150.0, 700.0), True), size, 3, label_dim=10).to(DEV)
    call = lambda z: vaw_amd.dpm_sample(net, z, class_labels=y, num_steps=5, **SOLVERS[solver])
    z = torch.randn(3, 3, size, size, device=DEV)
    torch.manual_seed(1)
    first = call(z)                                              # builds and caches the table (reads it back once)
    torch.cuda.synchronize()
    torch.manual_seed(1)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = call(z)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, second)


# ---- Sampler: captured graph ---------------------------------------------------------------------------------------------------
def test_sampler_hip_graph_returns_the_bytes_and_labels_of_the_eager_run():
    st = dict(guidance_scale=1.8, interval=(150.0, 700.0), solver="dpmpp2m_sde", sample_steps=5)
    model, size = model_for("dit", True)
    runs = []
    for graph in (False, True):
        args = sampler_args("edm", st, cpu_rng=False, hip_graph=graph, eta=0.8)
        torch.manual_seed(31)
        runs.append(vaw_amd.Sampler(args, torch.device(DEV), model, None).sample(9, 3, size, 10))
    (ei, el), (gi, gl) = runs
    assert len(ei) == len(gi) == len(el) == len(gl) == 3
    for b in range(3):
        assert gi[b].dtype.name == "uint8" and gi[b].shape == (3, size, size, 3)
        assert (gl[b] == el[b]).all() and (gi[b] == ei[b]).all(), f"batch {b}: {int((gi[b] != ei[b]).sum())} bytes differ"
    assert len({a.tobytes() for a in ei}) == 3          # three different batches, not one replayed output

"""The fused EDM / flow solver steps on the GPU (vaw_edm_input, vaw_edm_step, vaw_flow_step): each kernel kind bitwise the
tensor composition it replaces, the loops with `fused=True` bitwise `fused=False` from the same seed (tiny DiT, tiny UNet,
guidance always / in an interval / off), no host synchronisation once the tables are cached, and Sampler's captured graph."""
import itertools

import pytest
import torch

from conftest import perturb_
from sampler_cases import sampler_args

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops, samplers
from vaw_amd.gaussian_diffusion import ModelMeanType

DEV = "cuda"
SHAPES = [(2, 3, 8, 8), (1, 1, 5, 7), (3, 4, 32, 32)]          # 192 a row; 35: odd row, scalar path; 4096: four blocks a row
SHAPE_IDS = ["2x3x8x8", "1x1x5x7", "3x4x32x32"]
LAYOUTS = ["dense", "slice", "shifted"]
SCALE = 2.5


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


# ---- EDM kernels ----------------------------------------------------------------------------------------------------------
class Table:
    """An EDM table on the device with s(t) != 1 (vp scaling: the divisions are real) and churn on some steps only."""
    _made = {}

    @classmethod
    def get(cls, pred_type, batch):
        if (pred_type, batch) not in cls._made:
            net = vaw_amd.EDMDenoiser(torch.nn.Identity(), 8, 3, pred_type=pred_type).to(DEV)
            lo, hi = samplers._edm_sigma_range(net, "edm", None, None, 1e-3)
            tab = samplers._edm_tables(net, torch.device(DEV), batch, 6, lo, hi, 7, "heun", "edm", "vp", "vp", 1e-3, 1, 40, 0.05, 50.0, 1.003)
            assert any(tab.noise_on) and not all(tab.noise_on[:5])
            cls._made[pred_type, batch] = tab
        return cls._made[pred_type, batch]


def edm_eval_scalars(tab, i, mid):
    r = tab.coef[i, 14 if mid else 2:]
    return dict(s=r[0], sigma=r[1].float().reshape(1, 1, 1, 1), k1=r[5], k2=r[6])


def edm_slope(pred_type, ev, x, o):
    """_Path.slope of EDMDenoiser.forward's denoised image, with the evaluation's scalars as 0-dim device tensors."""
    sigma = ev["sigma"]
    c_in = 1 / (sigma ** 2 + 1).sqrt()
    x32 = (x / ev["s"]).to(torch.float32)
    den = {"EPSILON": lambda: x32 - sigma * o, "START_X": lambda: o, "VELOCITY": lambda: c_in ** 2 * x32 - sigma * c_in * o}[pred_type]()
    return ev["k1"] * x - ev["k2"] * den.to(torch.float64)


def edm_model_in(ev, x):
    sigma = ev["sigma"]
    c_in = 1 / (sigma ** 2 + 1).sqrt()
    return c_in * (x / ev["s"]).to(torch.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_edm_input_is_bitwise_the_tensor_composition(shape):
    N = shape[0]
    tab = Table.get("EPSILON", N)
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 30).to(DEV)
    nz = torch.randn(shape, generator=g, dtype=torch.float64).to(DEV)
    on, off = tab.noise_on.index(True), tab.noise_on.index(False)
    assert tab.host[on][1] != 0 and tab.host[off][1] == 0
    for i, stacked in itertools.product((on, off), (True, False)):
        ref_hat = tab.coef[i, 0] * x + tab.coef[i, 1] * nz          # (the product with a zero coefficient adds nothing)
        ref_in = edm_model_in(edm_eval_scalars(tab, i, False), ref_hat)
        buf = torch.full((2 * N if stacked else N, *shape[1:]), 7.0, device=DEV)
        x_hat = torch.empty_like(x)
        ops.edm_input(x, nz if tab.noise_on[i] else None, tab.coef, i, x_hat, buf[:N], buf[N:] if stacked else None)
        assert x_hat.dtype == torch.float64 and torch.equal(x_hat, ref_hat), (i, differ(x_hat, ref_hat))
        assert torch.equal(buf[:N], ref_in), (i, differ(buf[:N], ref_in))
        assert not stacked or torch.equal(buf[N:], ref_in)
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view(shape)          # scalar path on a misaligned destination
    ops.edm_input(x, nz, tab.coef, on, x_hat, shifted)
    assert torch.equal(shifted, edm_model_in(edm_eval_scalars(tab, on, False), tab.coef[on, 0] * x + tab.coef[on, 1] * nz))
    with pytest.raises(vaw_amd.VawError, match="row 6 outside"):
        ops.edm_input(x, nz, tab.coef, 6, x_hat, shifted)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_edm_step_kinds_are_bitwise_the_tensor_composition(shape, layout):
    N = shape[0]
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x_hat = (torch.randn(shape, generator=g, dtype=torch.float64) * 20).to(DEV)
    d_prev = torch.randn(shape, generator=g, dtype=torch.float64).to(DEV)
    out = model_output(shape, layout, 11 + len(layout))
    for pred_type, guided, i in itertools.product(ops.EDM_PRED, (True, False), (0, 3)):
        tab = Table.get(pred_type, N)
        what = (pred_type, guided, i)
        cond, uncond = out[:N], (out[N:] if guided else None)
        o = uncond + SCALE * (cond - uncond) if guided else cond
        hat, mid = edm_eval_scalars(tab, i, False), edm_eval_scalars(tab, i, True)
        h, ah, w1, w2 = tab.coef[i, 10], tab.coef[i, 11], tab.coef[i, 12], tab.coef[i, 13]
        d_cur = edm_slope(pred_type, hat, x_hat, o)
        # Euler
        got = ops.edm_step(ops.STEP_EULER, pred_type, cond, uncond, SCALE, x_hat, None, tab.coef, i, x_out=torch.empty_like(x_hat))
        ref = x_hat + h * d_cur
        assert got.dtype == torch.float64 and torch.equal(got, ref), (what, "euler", differ(got, ref))
        # Heun, prediction: d_cur and the midpoint's network input, into both halves of a stacked buffer
        buf = torch.full((2 * N, *shape[1:]), 7.0, device=DEV)
        d_got = ops.edm_step(ops.STEP_PREDICT, pred_type, cond, uncond, SCALE, x_hat, torch.empty_like(x_hat), tab.coef, i,
                             model_in=buf[:N], model_in_dup=buf[N:])
        x_mid = x_hat + ah * d_cur
        ref_in = edm_model_in(mid, x_mid)
        assert torch.equal(d_got, d_cur), (what, "d_cur", differ(d_got, d_cur))
        assert torch.equal(buf[:N], ref_in) and torch.equal(buf[N:], ref_in), (what, "midpoint input", differ(buf[:N], ref_in))
        # Heun, correction, from a d_cur of its own
        x_mid = x_hat + ah * d_prev
        ref = x_hat + h * (w1 * d_prev + w2 * edm_slope(pred_type, mid, x_mid, o))
        got = ops.edm_step(ops.STEP_CORRECT, pred_type, cond, uncond, SCALE, x_hat, d_prev, tab.coef, i, x_out=torch.empty_like(x_hat))
        assert torch.equal(got, ref), (what, "correct", differ(got, ref))
        assert bool(torch.isfinite(ref).all())


# ---- flow kernel -----------------------------------------------------------------------------------------------------------
def flow_fm(path_type, mean_type):
    return vaw_amd.FlowMatching(args=sampler_args("flow", dict(guidance_scale=1.0), path_type=path_type), model_mean_type=ModelMeanType[mean_type])


def flow_drift(fm, out, x, t, sde):
    _, s, _, ds = fm.interpolant(t)
    g2 = 2 * s * ds
    v, score = samplers._flow_fields(fm, out, x, t)
    return (v - 0.5 * g2 * score if sde else v), g2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_flow_step_kinds_are_bitwise_the_tensor_composition(shape, layout):
    N, steps, k = shape[0], 6, 2          # step 2 of 5: t well inside (0, 1), every interpolant coefficient generic
    g = torch.Generator().manual_seed(sum(shape) + 2)
    x = torch.randn(shape, generator=g).to(DEV)
    nz = torch.randn(shape, generator=g).to(DEV)
    f_prev = torch.randn(shape, generator=g).to(DEV)
    kick_prev = (torch.randn(shape, generator=g) * 0.3).to(DEV)
    x_pred = torch.randn(shape, generator=g).to(DEV)
    out = model_output(shape, layout, 23 + len(layout))
    grids = {True: torch.cat([torch.linspace(1.0, 0.04, steps, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)]),
             False: torch.linspace(1.0, 0.0, steps, device=DEV)}
    for (mean_type, path_type), sde, guided in itertools.product(zip(ops.FLOW_MEAN, ("cosine", "linear", "cosine", "linear_logsnr")),
                                                                 (True, False), (True, False)):
        fm = flow_fm(path_type, mean_type)
        tab = samplers._flow_tables(fm, "sde" if sde else "ode", "heun", steps, N, torch.device(DEV))
        what = (mean_type, path_type, sde, guided)
        e0, e1, grid = 2 * k, 2 * k + 1, grids[sde]
        dt = grid[k + 1] - grid[k]
        t0, t1 = (fm.expand_t_like_x(grid[j], x) for j in (k, k + 1))
        assert torch.equal(tab.times[e0, :N], t0.view(N)) and torch.equal(tab.times[e1, N:], t1.view(N))
        cond, uncond = out[:N], (out[N:] if guided else None)
        o = uncond + SCALE * (cond - uncond) if guided else cond
        f0, g2 = flow_drift(fm, o, x, t0, sde)
        kick = torch.sqrt(g2) * nz * torch.sqrt(torch.abs(dt)) if sde else None
        euler = x + f0 * dt + kick if sde else x + dt * f0
        new = lambda rows=N: torch.full((rows, *shape[1:]), 7.0, device=DEV)
        # Euler
        got = ops.flow_step(ops.STEP_EULER, sde, mean_type, cond, uncond, SCALE, x, nz if sde else None, None, None, None, tab.coef, e0, e0, new())
        assert got.dtype == torch.float32 and torch.equal(got, euler), (what, "euler", differ(got, euler))
        if sde:          # the noise-free last step
            got = ops.flow_step(ops.STEP_EULER, True, mean_type, cond, uncond, SCALE, x, None, None, None, None, tab.coef, e0, e0, new())
            assert torch.equal(got, x + f0 * dt), (what, "last", differ(got, x + f0 * dt))
        # Heun, prediction (into both halves of a stacked buffer)
        buf, f_got, k_got = new(2 * N), new(), (new() if sde else None)
        ops.flow_step(ops.STEP_PREDICT, sde, mean_type, cond, uncond, SCALE, x, nz if sde else None, None, f_got, k_got, tab.coef, e0, e1,
                      buf[:N], buf[N:])
        assert torch.equal(buf[:N], euler) and torch.equal(buf[N:], euler), (what, "predict", differ(buf[:N], euler))
        assert torch.equal(f_got, f0), (what, "f0", differ(f_got, f0))
        assert not sde or torch.equal(k_got, kick), (what, "kick")
        # Heun, correction
        f1, _ = flow_drift(fm, o, x_pred, t1, sde)
        ref = x + 0.5 * (f_prev + f1) * dt + kick_prev if sde else x + 0.5 * dt * (f_prev + f1)
        got = ops.flow_step(ops.STEP_CORRECT, sde, mean_type, cond, uncond, SCALE, x, None, x_pred, f_prev, kick_prev if sde else None, tab.coef,
                            e0, e1, new())
        assert torch.equal(got, ref), (what, "correct", differ(got, ref))
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(euler).all())


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


def both_ways(fn, shape, **kw):
    """fn with fused=False and fused=True from one seed: (composition, fused), each followed by one more draw of the stream."""
    res = []
    for fused in (False, True):
        torch.manual_seed(11)
        x = fn(torch.randn(shape, device=DEV), fused=fused, **kw)
        res.append((x, torch.randn(4, device=DEV)))
    (ref, ref_next), (got, got_next) = res
    assert got.dtype == ref.dtype and got.shape == ref.shape and bool(torch.isfinite(ref).all())
    assert torch.equal(got, ref), differ(got, ref)
    assert torch.equal(got_next, ref_next), "the generator was left at another offset"
    return ref


@pytest.mark.parametrize("guidance", list(GUIDANCE))
@pytest.mark.parametrize("solver,S_churn", [("heun", 0), ("heun", 40), ("euler", 40)])
@pytest.mark.parametrize("name", ["dit", "unet"])
def test_edm_sample_fused_is_bitwise_the_composition(name, solver, S_churn, guidance):
    model, size = model_for(name, True)
    scale, interval = GUIDANCE[guidance]
    calls = []
    cfg = vaw_amd.IntervalCFG(model, 10, scale, interval, True)
    model.register_forward_pre_hook(lambda m, a: calls.append(a[0].shape[0]))
    net = vaw_amd.EDMDenoiser(cfg, size, 3, pred_type="EPSILON" if name == "dit" else "VELOCITY", label_dim=10).to(DEV)
    y = torch.tensor([1, 5, 9], device=DEV)
    try:
        ref = both_ways(lambda z, **kw: vaw_amd.edm_sample(net, z, class_labels=y, num_steps=5, solver=solver, S_churn=S_churn, S_min=0.05,
                                                           S_max=50.0, **kw), (3, 3, size, size))
    finally:
        model._forward_pre_hooks.clear()
    assert ref.dtype == torch.float64
    half = len(calls) // 2
    assert calls[:half] == calls[half:] and half == (9 if solver == "heun" else 5)          # the same calls, guided at the same evaluations
    stacked = sum(b == 6 for b in calls[:half])
    assert stacked == {"always": half, "off": 0}.get(guidance, stacked) and (guidance != "interval" or 0 < stacked < half)


@pytest.mark.parametrize("guidance", ["always", "interval"])
@pytest.mark.parametrize("solver", ["heun", "euler"])
@pytest.mark.parametrize("kind", ["sde", "ode"])
@pytest.mark.parametrize("name", ["dit", "unet"])
def test_flow_samplers_fused_are_bitwise_the_composition(name, kind, solver, guidance):
    model, size = model_for(name, False)
    scale, interval = {"always": (SCALE, (-1.0, -1.0)), "interval": (1.8, (0.2, 0.7))}[guidance]
    cfg = vaw_amd.IntervalCFG(model, 10, scale, interval, True)
    fm = flow_fm("linear", "VELOCITY" if name == "dit" else "VECTOR")          # (the two that are finite at both ends of the linear path)
    y = torch.tensor([1, 5, 9], device=DEV)
    fn = vaw_amd.flow_sde_sample if kind == "sde" else vaw_amd.flow_ode_sample
    ref = both_ways(lambda z, **kw: fn(fm, cfg, z, num_steps=5, solver=solver, y=y, **kw), (3, 3, size, size))
    assert ref.dtype == torch.float32
    tab = samplers._flow_tables(fm, kind, solver, 5, 3, torch.device(DEV))
    active = [cfg.guidance_active(t) for t in tab.t_mean]
    assert all(active) if guidance == "always" else 0 < sum(active) < len(active)


def test_fused_true_refuses_what_is_not_fused():
    fm = flow_fm("linear", "VELOCITY")
    z = torch.randn(3, 3, 8, 8, device=DEV)
    model = lambda x, t, **kw: x
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.flow_ode_sample(fm, model, z, num_steps=4, solver="rk4", fused=True)
    with pytest.raises(ValueError, match="fused=True"):
        vaw_amd.flow_sde_sample(flow_fm("linear", "SCORE"), model, z, num_steps=4, fused=True)
    with pytest.raises(NotImplementedError, match="dopri5"):
        vaw_amd.flow_ode_sample(fm, model, z, solver="dopri5", fused=True)
    for solver in ("midpoint", "rk4"):          # fused=None: the tensor composition, as before
        assert torch.equal(vaw_amd.flow_ode_sample(fm, model, z, num_steps=4, solver=solver),
                           vaw_amd.flow_ode_sample(fm, model, z, num_steps=4, solver=solver, fused=False))


# ---- no host synchronisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edm_heun_churn", "flow_sde_heun", "flow_ode_euler"])
def test_second_call_does_not_synchronise_with_the_host(which):
    y = torch.tensor([1, 5, 9], device=DEV)
    if which.startswith("edm"):
        model, size = model_for("dit", True)
        net = vaw_amd.EDMDenoiser(vaw_amd.IntervalCFG(model, 10, 1.8, (150.0, 700.0), True), size, 3, label_dim=10).to(DEV)
        call = lambda z: vaw_amd.edm_sample(net, z, class_labels=y, num_steps=5, S_churn=40, S_min=0.05, S_max=50.0)
    else:
        model, size = model_for("dit", False)
        cfg, fm = vaw_amd.IntervalCFG(model, 10, 1.8, (0.2, 0.7), True), flow_fm("linear", "VELOCITY")
        if "sde" in which:
            call = lambda z: vaw_amd.flow_sde_sample(fm, cfg, z, num_steps=5, solver="heun", y=y)
        else:
            call = lambda z: vaw_amd.flow_ode_sample(fm, cfg, z, num_steps=5, solver="euler", y=y)
    z = torch.randn(3, 3, size, size, device=DEV)
    torch.manual_seed(1)
    first = call(z)                                              # builds and caches the tables (reads them back once)
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
@pytest.mark.parametrize("case", ["edm_heun", "flow_sde_heun"])
def test_sampler_hip_graph_returns_the_bytes_and_labels_of_the_eager_run(case):
    if case == "edm_heun":
        kind, st, (model, size) = "edm", dict(guidance_scale=1.8, interval=(150.0, 700.0), solver="heun", sample_steps=5), model_for("dit", True)
        diff = None
    else:
        kind, st = "flow", dict(guidance_scale=1.8, interval=(0.2, 0.7), solver="heun", sample_steps=5, path_type="linear", mean_type="VELOCITY")
        model, size = model_for("dit", False)
    runs = []
    for graph in (False, True):
        args = sampler_args(kind, st, cpu_rng=False, hip_graph=graph)
        if kind == "flow":
            diff = vaw_amd.FlowMatching(args=args, model_mean_type=ModelMeanType.VELOCITY)
        torch.manual_seed(31)
        images, labels = vaw_amd.Sampler(args, torch.device(DEV), model, diff).sample(9, 3, size, 10)
        runs.append((images, labels))
    (ei, el), (gi, gl) = runs
    assert len(ei) == len(gi) == len(el) == len(gl) == 3
    for b in range(3):
        assert gi[b].dtype.name == "uint8" and gi[b].shape == (3, size, size, 3)
        assert (gl[b] == el[b]).all() and (gi[b] == ei[b]).all(), f"batch {b}: {int((gi[b] != ei[b]).sum())} bytes differ"
    assert len({a.tobytes() for a in ei}) == 3          # three different batches, not one replayed output

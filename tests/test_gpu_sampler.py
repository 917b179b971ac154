"""The sampler on the HIP path: the fused guided reverse step (vaw_guided_sample_step), the guidance combination
(vaw_cfg_combine), the uint8 image finish (vaw_finish_images), the loops with the guidance interval decided on the host, and
vaw_amd.Sampler end to end against tests/golden/sampler.pt (the unmodified reference's Sampler.sample on CPU)."""
import math

import pytest
import torch

from conftest import load_pt, perturb_, sampling_model, sampling_model_2c
from sampler_cases import Standin, build, in_band, sampler_args, spaced

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops

DEV = "cuda"
SHAPES = [(3, 8, 8), (193,), (4, 32, 32), (3, 64, 64)]
SHAPE_IDS = ["n192", "n193", "n4096", "n12288"]
MODES = [(mt, vt) for mt in ("EPSILON", "PREVIOUS_X") for vt in ("FIXED_SMALL", "LEARNED", "LEARNED_RANGE")]
KEYS = ("sample", "pred_xstart", "mean", "log_variance")


def diffusion(mt, vt):
    wt = "constant" if mt == "PREVIOUS_X" else "lambda"          # 'lambda' has no PREVIOUS_X weight (training side only)
    return vaw_amd.GaussianDiffusion(args=sampler_args("ddim", dict(guidance_scale=2.5), weight_type=wt), betas=vaw_amd.get_named_beta_schedule("linear", 100),
                                     model_mean_type=vaw_amd.ModelMeanType[mt], model_var_type=vaw_amd.ModelVarType[vt],
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=False)


def step_inputs(shape, learned, seed, N=3, layout="plain"):
    """x, noise and one stacked [2N, (2)C, ...] model output on the device.  layout: plain | shifted (base pointer one float
    past a 16-byte boundary) | ld_odd (rows 2 floats further apart than their length: model_ld % 4 == 2)."""
    g = torch.Generator().manual_seed(seed)
    k = 2 if learned else 1
    oshape = (2 * N, k * shape[0], *shape[1:])
    vals = torch.randn(oshape, generator=g) * 0.7
    if learned:
        vals[:, shape[0]:] = torch.rand((2 * N, *shape), generator=g) * 2 - 1
    row = vals[0].numel()
    if layout == "shifted":
        buf = torch.empty(vals.numel() + 1, device=DEV)
        out = buf[1:].view(oshape)
    elif layout == "ld_odd":
        buf = torch.empty(2 * N, row + 2, device=DEV)
        out = buf[:, :row].view(oshape)
    else:
        out = torch.empty(oshape, device=DEV)
    out.copy_(vals)
    x = torch.randn((N, *shape), generator=g).to(DEV)
    nz = torch.randn((N, *shape), generator=g).to(DEV)
    return out, x, nz


def quarters(out, N, C, learned):
    cond, uncond = out[:N], out[N:]
    return cond[:, :C], uncond[:, :C], (cond[:, C:] if learned else None), (uncond[:, C:] if learned else None)


def composition(out, N, C, learned, scale, kind, x, nz, coef, mean_mode, var_mode, clip, eta):
    """What the parent commit runs: IntervalCFG's three tensor operations, the split made contiguous, vaw_sample_step."""
    with_label, without = out[:N], out[N:]
    comb = without + scale * (with_label - without)
    m, v = (torch.split(comb, C, dim=1) if learned else (comb, None))
    return ops.sample_step(kind, m.contiguous(), None if v is None else v.contiguous(), x, nz if kind else None, coef, mean_mode,
                           var_mode, clip, eta, want_all=True), comb


def restate(comb, x, nz, coef, kind, mean_mode, var_mode, clip, eta, C, dtype):
    """The reference's p_mean_variance + p_sample / ddim_sample formulas in torch on the CPU, in `dtype`."""
    B = x.shape[0]
    comb, x, nz = (a.detach().cpu().to(dtype) for a in (comb, x, nz))
    m = comb[:, :C].flatten(1)
    x, nz = x.flatten(1), nz.flatten(1)
    c = [coef.detach().cpu()[:, i:i + 1].to(dtype) for i in range(16)]
    pred = c[0] * x + c[1] * m
    if clip:
        pred = pred.clamp(-1, 1)
    if var_mode == 0:
        lv = c[5].expand_as(x)
    else:
        v = comb[:, C:].flatten(1)
        lv = v if var_mode == 1 else ((v + 1) / 2) * c[5] + (1 - (v + 1) / 2) * c[4]
    mean = m if mean_mode == 1 else c[2] * pred + c[3] * x
    mask = (c[11] == 0).to(dtype)
    res = {"pred_xstart": pred, "mean": mean, "log_variance": lv}
    if kind == 1:
        res["sample"] = mean + mask * torch.exp(0.5 * lv) * nz
    elif kind == 2:
        eps = (c[6] * x - pred) / c[7]
        sigma = eta * c[9] * c[12]
        res["sample"] = pred * c[8] + torch.sqrt(1 - c[10] - sigma ** 2) * eps + mask * sigma * nz
    return {k: v.reshape(B, -1) for k, v in res.items()}


def close(got, exp, what, extra):
    """The tolerance of test_bpd_terms_kernel_vs_float64: 1e-4 relative + 1e-5 of the largest expected value + twice what
    the same formulas cost in f32 (torch on the CPU) against float64.  Prints the figures first."""
    got, exp = got.detach().double().cpu().reshape(exp.shape), exp.double()
    scale = float(exp.abs().max())
    err = (got - exp).abs()
    allow = 1e-4 * exp.abs() + 1e-5 * scale + extra
    print(f"{what}: max|err| = {float(err.max()):.3e}  max|expected| = {scale:.3e}  worst err/allowed = {float((err / allow).max()):.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= allow).all()), f"{what}: max|err| {float(err.max()):.3e}"


def run_step_cases(shape, check):
    N, C = 3, shape[0]
    for i, (mt, vt) in enumerate(MODES):
        d = diffusion(mt, vt)
        learned = vt.startswith("LEARNED")
        mean_mode, var_mode = int(mt == "PREVIOUS_X"), {"LEARNED": 1, "LEARNED_RANGE": 2}.get(vt, 0)
        out, x, nz = step_inputs(shape, learned, 40 + i)
        coef = d._sample_rows(torch.tensor([0, 99, 37], device=DEV))          # a t = 0 row among t > 0 rows
        for kind, eta in ((0, 0.0), (1, 0.0), (2, 0.7)):
            for clip in (True, False):
                for scale in (2.5, 1.0):
                    got = ops.guided_sample_step(kind, *quarters(out, N, C, learned), scale, x, nz if kind else None, coef,
                                                 mean_mode, var_mode, clip, eta, want_all=True)
                    check(got, (out, N, C, learned, scale, kind, x, nz, coef, mean_mode, var_mode, clip, eta),
                          f"{mt}/{vt}/kind={kind}/clip={clip}/s={scale}/n={math.prod(shape)}")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_guided_step_is_bitwise_the_torch_combination_then_sample_step(shape):
    def check(got, a, what):
        ref, _ = composition(*a)
        assert set(got) == set(ref) == set(KEYS[0 if a[5] else 1:])
        for k in ref:
            assert torch.equal(got[k], ref[k]), f"{what}/{k}: {int((got[k] != ref[k]).sum())} elements differ"

    run_step_cases(shape, check)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_guided_step_vs_float64(shape):
    def check(got, a, what):
        out, N, C, learned, scale, kind, x, nz, coef, mean_mode, var_mode, clip, eta = a
        c64 = out.cpu().double()
        c64 = c64[N:] + scale * (c64[:N] - c64[N:])
        c32 = out.cpu()
        c32 = c32[N:] + scale * (c32[:N] - c32[N:])
        r64 = restate(c64, x, nz, coef, kind, mean_mode, var_mode, clip, eta, C, torch.float64)
        r32 = restate(c32, x, nz, coef, kind, mean_mode, var_mode, clip, eta, C, torch.float32)
        for k in r64:
            close(got[k], r64[k], f"{what}/{k}", extra=2 * (r32[k].double() - r64[k]).abs())

    run_step_cases(shape, check)


@pytest.mark.parametrize("layout", ["shifted", "ld_odd"])
def test_guided_step_scalar_path_on_a_misaligned_base_and_an_odd_row_distance(layout):
    shape, N, C = (3, 8, 8), 3, 3
    d = diffusion("EPSILON", "LEARNED_RANGE")
    out, x, nz = step_inputs(shape, True, 7, layout=layout)
    assert (out.data_ptr() % 16 != 0) if layout == "shifted" else (out.stride(0) % 4 == 2)
    coef = d._sample_rows(torch.tensor([0, 99, 37], device=DEV))
    for kind, eta in ((1, 0.0), (2, 0.7)):
        got = ops.guided_sample_step(kind, *quarters(out, N, C, True), 2.5, x, nz, coef, 0, 2, True, eta, want_all=True)
        ref, _ = composition(out, N, C, True, 2.5, kind, x, nz, coef, 0, 2, True, eta)
        for k in ref:
            assert torch.equal(got[k], ref[k]), f"{layout}/kind={kind}/{k}"


def test_sample_step_reads_split_halves_in_place_bitwise():
    d = diffusion("EPSILON", "LEARNED_RANGE")
    coef = d._sample_rows(torch.tensor([0, 99, 37], device=DEV))
    for shape in SHAPES:
        out, x, nz = step_inputs(shape, True, 11)
        m, v = torch.split(out[:3], shape[0], dim=1)
        assert not m.is_contiguous()
        for kind, vm in ((0, 2), (1, 1), (2, 2)):
            a = ops.sample_step(kind, m, v, x, nz if kind else None, coef, 0, vm, True, 0.3, want_all=True)
            b = ops.sample_step(kind, m.contiguous(), v.contiguous(), x, nz if kind else None, coef, 0, vm, True, 0.3, want_all=True)
            for k in b:
                assert torch.equal(a[k], b[k]), (shape, kind, k)


@pytest.mark.parametrize("n", [192, 193, 4096])
def test_cfg_combine_is_bitwise_the_three_torch_ops(n):
    g = torch.Generator().manual_seed(n)
    out = (torch.randn(6, n, generator=g) * 3).to(DEV)
    for scale in (2.5, 1.0, 1.3, -0.7):
        ref = out[3:] + scale * (out[:3] - out[3:])
        assert torch.equal(ops.cfg_combine(out[:3], out[3:], scale), ref), scale
    wide = torch.randn(6, 2 * n + 2, generator=g).to(DEV)             # rows further apart than their length
    ref = wide[3:, :n] + 2.5 * (wide[:3, :n] - wide[3:, :n])
    assert torch.equal(ops.cfg_combine(wide[:3, :n], wide[3:, :n], 2.5), ref)
    cfg = vaw_amd.IntervalCFG(lambda x, t, **kw: x, 10, 2.5)
    assert torch.equal(cfg.combine(out), out[3:] + 2.5 * (out[:3] - out[3:]))


def finish_ref(x):
    return ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 1, 5, 7), (3, 4, 32, 32), (2, 3, 64, 64), (1, 2, 3, 3)], ids=lambda s: "x".join(map(str, s)))
def test_finish_images_is_bitwise_the_torch_expression(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.rand(shape, generator=g, dtype=torch.float64) * 3 - 1.5).to(dtype)
    flat = x.flatten()
    special = torch.cat([torch.tensor([-1.0, 1.0], dtype=torch.float64), torch.arange(0, 256, dtype=torch.float64) / 127.5 - 1]).to(dtype)
    k = min(flat.numel() // 2, special.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:k]] = special[torch.randperm(special.numel(), generator=g)[:k]]
    x = x.to(DEV)
    ref = finish_ref(x)
    got = ops.finish_images(x)
    B, Cn, H, W = shape
    assert got.dtype == torch.uint8 and got.shape == (B, H, W, Cn) and got.is_contiguous()
    assert torch.equal(got, ref), f"{int((got != ref).sum())} bytes differ"
    # a destination one byte past a word boundary, guarded on both sides
    buf = torch.full((ref.numel() + 9,), 77, dtype=torch.uint8, device=DEV)
    dst = buf[5:5 + ref.numel()].view(ref.shape)
    assert dst.data_ptr() % 4 == 1
    assert ops.finish_images(x, out=dst) is dst and torch.equal(dst, ref)
    assert bool((buf[:5] == 77).all()) and bool((buf[5 + ref.numel():] == 77).all())
    # NaN writes 0
    xn = x.clone()
    xn.flatten()[::5] = float("nan")
    exp = ref.clone()
    exp.permute(0, 3, 1, 2)[torch.isnan(xn)] = 0
    assert torch.equal(ops.finish_images(xn), exp)


class Recorder:
    """Stand-in denoiser that records the batch size of every call."""

    def __init__(self, fn):
        self.fn, self.batches = fn, []

    def __call__(self, x, t, **kw):
        self.batches.append(x.shape[0])
        return self.fn(x, t, **kw)


@pytest.mark.parametrize("interval", [(-1.0, -1.0), (200.0, 700.0)], ids=["always", "interval"])
@pytest.mark.parametrize("kind", ["ddim", "p"])
def test_loops_with_interval_cfg_are_bitwise_the_parent_composition(kind, interval):
    """ddim_sample_loop / p_sample_loop over a 10-step respaced chain with an IntervalCFG model: bitwise the loop composed
    from the torch combination and ops.sample_step, with guidance switched exactly at the steps the host predicate names."""
    N, C, scale, eta = 3, 3, 2.5, (0.7 if kind == "ddim" else 0.0)
    d, _ = spaced("ddim10_eps_range_eta", sampler_args("ddim", dict(guidance_scale=scale)))
    assert d.num_timesteps == 10
    y = torch.tensor([1, 5, 9], device=DEV)
    rec = Recorder(sampling_model_2c)
    cfg = vaw_amd.IntervalCFG(rec, 10, scale, interval, True)
    torch.manual_seed(5)
    loop = d.ddim_sample_loop if kind == "ddim" else d.p_sample_loop
    got = loop(cfg, (N, C, 8, 8), model_kwargs={"y": y}, device=DEV, **({"eta": eta} if kind == "ddim" else {}))
    # the composition
    torch.manual_seed(5)
    x = torch.randn(N, C, 8, 8).to(DEV)
    expected_batches = []
    for i in reversed(range(10)):
        t = torch.full((N,), i, device=DEV, dtype=torch.long)
        tm = torch.full((N,), float(d.timestep_map[i]), device=DEV)
        guided = cfg.guidance_active(d._host_model_time(i))
        assert guided == cfg.guidance_active(float(d.timestep_map[i]))
        expected_batches.append(2 * N if guided else N)
        if guided:
            out = sampling_model_2c(x.repeat(2, 1, 1, 1), tm.repeat(2), y=torch.cat((y, torch.full_like(y, 10))))
            out = out[N:] + scale * (out[:N] - out[N:])
        else:
            out = sampling_model_2c(x, tm, y=y)
        m, v = torch.split(out, C, dim=1)
        noise = torch.randn(N, C, 8, 8).to(DEV)
        x = ops.sample_step(2 if kind == "ddim" else 1, m.contiguous(), v.contiguous(), x, noise, d._sample_rows(t), 0, 2, True, eta)["sample"]
    assert rec.batches == expected_batches
    if interval[0] >= 0:
        assert 0 < sum(b == 2 * N for b in expected_batches) < 10          # active for part of the chain only
    assert torch.equal(got, x), f"{int((got != x).sum())} elements differ"


def run_sampler(kind, st, seed, g, cls=None, **kw):
    args = sampler_args(kind, st)
    diff, model = build(kind, st, args)
    s = (cls or vaw_amd.Sampler)(args, torch.device(DEV), model, diff, **kw)
    floats, finish = [], s._inverse_normalize
    s._inverse_normalize = lambda x: (floats.append(x.detach().clone()), finish(x))[1]
    torch.manual_seed(seed)
    images, labels = s.sample(g["num_samples"], g["sample_size"], g["image_size"], g["num_classes"])
    return images, labels, floats


CASE_NAMES = ["p20_x0_large/always", "p20_x0_large/interval", "ddim10_eps_range_eta/always", "ddim10_eps_range_eta/interval", "edm_heun",
              "edm_euler", "flow_sde_heun"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_sampler_sample_vs_reference_golden(name):
    """Sampler.sample on the GPU under the CPU RNG stream against the unmodified reference's.  Labels equal; float samples
    within rtol / atol 1e-4 for DDIM and 1e-5 / 1e-6 for EDM and flow; bytes equal except where the fixture's value lies in the
    boundary band of tests/golden/SAMPLER.md, where one level is allowed."""
    g = load_pt("sampler.pt")
    assert list(g["cases"]) == CASE_NAMES
    rec = g["cases"][name]
    kind = rec["kind"]
    images, labels, floats = run_sampler(kind, rec["settings"], rec["seed"], g)
    assert isinstance(images, list) and isinstance(labels, list) and len(images) == len(labels) == len(floats) == 2
    rtol, atol = (1e-4, 1e-4) if kind == "ddim" else (1e-5, 1e-6)
    for b in range(2):
        img, lab = images[b], labels[b]
        assert img.dtype.name == "uint8" and img.shape == (3, 8, 8, 3) and lab.dtype.name == "int64" and lab.shape == (3,)
        assert (lab == rec["labels"][b].numpy()).all()
        f, ef = floats[b].cpu(), rec["floats"][b]
        assert f.dtype == ef.dtype and f.shape == ef.shape
        err = (f - ef).abs()
        print(f"{name}[{b}]: float max|err| = {float(err.max()):.3e}  worst err/allowed = {float((err / (atol + rtol * ef.abs())).max()):.3f}")
        torch.testing.assert_close(f, ef, rtol=rtol, atol=atol)
        diff = (torch.from_numpy(img).int() - rec["images"][b].int()).abs()
        band = in_band(ef)
        print(f"{name}[{b}]: {int((diff != 0).sum())} of {diff.numel()} bytes differ, {int(band.sum())} in the boundary band")
        assert bool((diff[~band] == 0).all()) and bool((diff[band] <= 1).all())


def test_sampler_refusals():
    st = dict(guidance_scale=2.5)
    model = Standin(sampling_model)
    with pytest.raises(NotImplementedError, match="decode_fn"):
        vaw_amd.Sampler(sampler_args("ddim", st, in_chans=4), DEV, model, None)
    with pytest.raises(NotImplementedError, match="classifier"):
        vaw_amd.Sampler(sampler_args("ddim", st), DEV, model, None, classifier=object())
    with pytest.raises(ValueError, match="Unsupported model_mode"):
        vaw_amd.Sampler(sampler_args("ddim", st, model_mode="energy"), DEV, model, None).sample(3, 3, 8, 10)
    fst = dict(solver="dopri5", sample_steps=5, path_type="linear", mean_type="VELOCITY", guidance_scale=2.5)
    args = sampler_args("flow", fst, sampler_type="ode")
    fm, model = build("flow", fst, args)
    with pytest.raises(NotImplementedError, match="dopri5"):
        vaw_amd.Sampler(args, DEV, model, fm).sample(3, 3, 8, 10)
    args = sampler_args("flow", dict(fst, solver="heun"), sampler_type="ode")          # the fixed-grid ODE solvers do run
    images, labels = vaw_amd.Sampler(args, DEV, model, build("flow", fst, args)[0]).sample(3, 3, 8, 10)
    assert len(images) == 1 and images[0].shape == (3, 8, 8, 3) and images[0].dtype.name == "uint8"


class ParentCFG(torch.nn.Module):
    """IntervalCFG as the parent commit has it: three tensor operations, the predicate read back from the device, and no
    guided_halves -- so the reverse step takes the unfused route."""

    def __init__(self, model, num_classes, guidance_scale, interval, class_cond):
        super().__init__()
        self.model, self.null_label, self.guidance_scale = model, int(num_classes), float(guidance_scale)
        self.ref = vaw_amd.IntervalCFG(model, num_classes, guidance_scale, interval, class_cond)

    def forward(self, x, t, **kw):
        n, y = x.shape[0], kw.get("y")
        if not self.ref.guidance_active(float(t.float().mean())):
            return self.model(x, t, **kw)
        out = self.model(x.repeat(2, 1, 1, 1), t.repeat(2), **{**kw, "y": torch.cat((y, y.new_full(y.shape, self.null_label)))})
        out = out[0] if isinstance(out, tuple) else out
        return out[n:] + self.guidance_scale * (out[:n] - out[n:])


class UnfusedSampler(vaw_amd.Sampler):
    def _build_cfg_model(self, num_classes):
        return ParentCFG(self.model, num_classes, self.args.guidance_scale, self.args.interval, self.args.class_cond).eval()

    def _inverse_normalize(self, samples):
        return finish_ref(samples)


def test_tiny_dit_guided_ddim_sampler_equals_the_unfused_composition():
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.1, num_classes=10,
              learn_sigma=True)
    torch.manual_seed(3)
    model = vaw_amd.DiT(compute_dtype="fp32", **kw)
    perturb_(model, 17)
    model = model.to(DEV).eval()
    outs = []
    for cls in (vaw_amd.Sampler, UnfusedSampler):
        args = sampler_args("ddim", dict(guidance_scale=2.5, interval=(100.0, 900.0)), in_chans=4, learn_sigma=True)
        d = vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(1000, "5"), args=args, betas=vaw_amd.get_named_beta_schedule("linear", 1000),
                                    model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.LEARNED_RANGE,
                                    loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        s = cls(args, torch.device(DEV), model, d, decode_fn=lambda z: z[:, :3] * args.latent_scale)
        floats, finish = [], s._inverse_normalize
        s._inverse_normalize = lambda x: (floats.append(x.detach().clone()), finish(x))[1]
        torch.manual_seed(21)
        images, labels = s.sample(4, 4, 8, 10)
        assert len(floats) == 1 and floats[0].shape == (4, 3, 8, 8) and bool(torch.isfinite(floats[0]).all())
        assert len(images) == len(labels) == 1 and images[0].dtype.name == "uint8" and images[0].shape == (4, 8, 8, 3)
        outs.append((images[0], labels[0]))
    assert (outs[0][1] == outs[1][1]).all() and (outs[0][0] == outs[1][0]).all()
    assert len(set(outs[0][0].flatten().tolist())) > 8          # an image, not a constant

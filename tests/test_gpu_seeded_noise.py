"""Per-sample seeded noise on the GPU: vaw_randn_seeded against the numpy restatement (tests/seeded_noise_cases.py) -- words and
uniforms bitwise, normals within 4x what float32 arithmetic costs numpy, bf16 / float64 the conversions of the float32 value,
write bounds at every alignment, row independence, refusals -- and the samplers under args.sample_seed / SeededNoise: the
image of global index k bitwise the same at every batch size, on every shard, from every start, eagerly and from a captured
graph, fused and as the tensor composition.  The stand-in network is elementwise in x, so a row's image depends on its own row
alone, as in the t_chunk tests of calc_bpd_loop."""
import functools

import numpy as np
import pytest
import torch

import seeded_noise_cases as sc
from conftest import sampling_model
from sampler_cases import Standin, sampler_args

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd.noise import SeededNoise

DEV = "cuda"
PER_SAMPLE = [1, 3, 4, 5, 1023, 4100]
SEEDS = [0, 1, 2 ** 32, 2 ** 63 - 1, -1]
DRAWS = [0, 1, 2 ** 32 - 1]
N_MAX = max(PER_SAMPLE)
CANARY = 0xA5


def seed_rows(B):
    """The seed vectors of the kernel tests: every seed alone for B = 1, two triples that cover them all for B = 3."""
    return [[s] for s in SEEDS] if B == 1 else [SEEDS[:3], [SEEDS[3], SEEDS[4], SEEDS[0]]]


# the restatement, once per (seed, draw, tag) at the longest row: shorter rows are prefixes (test_seeded_noise_cpu.py)
@functools.lru_cache(maxsize=None)
def ref_bits(seed, draw, tag=sc.TAG_NOISE):
    return sc.bits(seed, draw, N_MAX, tag)


@functools.lru_cache(maxsize=None)
def ref_normal(seed, draw, dtype):
    return sc._box_muller(sc.uniform_of(ref_bits(seed, draw)), dtype)


@functools.lru_cache(maxsize=None)
def yardstick():
    """What evaluating the formula in float32 costs numpy against float64, over every (seed, draw) the tests use."""
    return max(float(np.abs(ref_normal(s, d, np.float32).astype(np.float64) - ref_normal(s, d, np.float64)).max()) for s in SEEDS for d in DRAWS)


def device_seeds(seeds):
    return torch.tensor(seeds, dtype=torch.int64, device=DEV)


def rows(fn, seeds, draw, n):
    return np.stack([fn(s, draw)[:n] for s in seeds])


# ---- the kernel against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", PER_SAMPLE)
def test_words_and_uniforms_are_bitwise_the_restatement(n, B):
    for seeds in seed_rows(B):
        st = device_seeds(seeds)
        for draw in DRAWS:
            for tag in (sc.TAG_NOISE, sc.TAG_LABELS):
                want = rows(functools.partial(ref_bits, tag=tag), seeds, draw, n)
                got = ops.randn_seeded(st, (B, n), draw, tag=tag, mode="bits")
                assert got.dtype == torch.int32 and got.shape == (B, n)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (seeds, draw, tag)
                u = ops.randn_seeded(st, (B, n), draw, tag=tag, mode="uniform")
                assert u.dtype == torch.float32
                assert np.array_equal(u.cpu().numpy().view(np.uint32), sc.uniform_of(want).view(np.uint32)), (seeds, draw, tag)
                assert float(u.min()) > 0.0 and float(u.max()) <= 1.0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", PER_SAMPLE)
def test_normals_vs_the_float64_restatement(n, B):
    """The bound: 4x the largest deviation of a numpy float32 evaluation of the same formula from float64 over the cases of this
    file (the device's logf and sincospif may each differ from numpy's by a few ulp)."""
    bound = 4 * yardstick()
    worst = 0.0
    for seeds in seed_rows(B):
        st = device_seeds(seeds)
        for draw in DRAWS:
            got = ops.randn_seeded(st, (B, n), draw)
            assert got.dtype == torch.float32 and got.shape == (B, n) and bool(torch.isfinite(got).all())
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - rows(lambda s, d: ref_normal(s, d, np.float64), seeds, draw, n)).max())
            worst = max(worst, err)
    print(f"n={n} B={B}: kernel max|err| vs float64 = {worst:.3e}; numpy float32 yardstick {yardstick():.3e}, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", PER_SAMPLE)
def test_bf16_and_float64_are_conversions_of_the_float32_value(n, B):
    for seeds in seed_rows(B):
        st = device_seeds(seeds)
        for draw in DRAWS:
            f32 = ops.randn_seeded(st, (B, n), draw)
            assert torch.equal(ops.randn_seeded(st, (B, n), draw, dtype=torch.bfloat16), f32.to(torch.bfloat16))
            f64 = ops.randn_seeded(st, torch.empty(B, n, dtype=torch.float64, device=DEV), draw)
            assert f64.dtype == torch.float64 and torch.equal(f64, f32.double())


KINDS = [("bits", torch.int32, (0, 4, 8)), ("uniform", torch.float32, (0, 4, 8)), ("normal", torch.float32, (0, 4, 8)),
         ("normal", torch.bfloat16, (0, 4, 8)), ("normal", torch.float64, (0, 8, 24))]


def guarded(dtype, shape, offset, pad=64):
    """(buffer of canary bytes, contiguous view of `shape` that starts `offset` bytes past a 16-byte boundary)."""
    nbytes = int(np.prod(shape)) * dtype.itemsize
    buf = torch.full((pad + nbytes + pad,), CANARY, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[pad + offset: pad + offset + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % 16 == offset % 16
    return buf, view, pad + offset, nbytes


@pytest.mark.parametrize("mode, dtype, offsets", KINDS, ids=[f"{m}-{str(d)[6:]}" for m, d, _ in KINDS])
def test_nothing_is_written_outside_the_output_at_any_alignment(mode, dtype, offsets):
    st = device_seeds(SEEDS[:3])
    for n in PER_SAMPLE:
        want = ops.randn_seeded(st, (3, n), 1, mode=mode, dtype=dtype)
        for off in offsets:
            buf, view, lo, nbytes = guarded(dtype, (3, n), off)
            assert ops.randn_seeded(st, (3, n), 1, mode=mode, dtype=dtype, out=view) is view
            assert torch.equal(view, want), (n, off)
            assert bool((buf[:lo] == CANARY).all()) and bool((buf[lo + nbytes:] == CANARY).all()), (n, off)


def test_rows_depend_on_their_own_seed_alone():
    a, b, c = 7, 2 ** 40 + 3, -5
    for n in PER_SAMPLE:
        for mode, dtype in (("bits", None), ("uniform", None), ("normal", torch.float32), ("normal", torch.float64), ("normal", torch.bfloat16)):
            draw = lambda seeds, m=n: ops.randn_seeded(device_seeds(seeds), (len(seeds), m), 3, mode=mode, dtype=dtype)
            together = draw([a, b, c])
            for i, s in enumerate((a, b, c)):
                assert torch.equal(together[i:i + 1], draw([s])), (n, mode, s)
            assert torch.equal(draw([c, a, b]), together[[2, 0, 1]])
            assert not torch.equal(together[0], together[1])
    for mode in ("bits", "uniform", "normal"):
        st = device_seeds([a, b, c])
        assert torch.equal(ops.randn_seeded(st, (3, 5), 3, mode=mode), ops.randn_seeded(st, (3, 8), 3, mode=mode)[:, :5])


def test_refused_calls_launch_nothing():
    lib = vaw_amd.lib()
    buf, view, _, _ = guarded(torch.float64, (2, 8), 0)
    st = device_seeds([1, 2])
    for call, word in sc.refused_calls(view.data_ptr(), st.data_ptr()):
        assert lib.vaw_randn_seeded(*call, torch.cuda.current_stream().cuda_stream) == -1, call
        assert word in lib.vaw_last_error_string().decode(), (call, word)
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and st.tolist() == [1, 2]
    for bad in (dict(mode="gauss"), dict(dtype=torch.float16), dict(mode="bits", dtype=torch.float32), dict(mode="uniform", dtype=torch.float64),
                dict(out=torch.empty(2, 9, device=DEV)), dict(out=torch.empty(2, 16, device=DEV)[:, ::2])):
        with pytest.raises(vaw_amd.VawError):
            ops.randn_seeded(st, (2, 8), 0, **bad)
    for seeds in (st[:1], st.int(), st.view(2, 1)):
        with pytest.raises(vaw_amd.VawError):
            ops.randn_seeded(seeds, (2, 8), 0)


def test_seeded_noise_draws_are_the_restatement():
    seeds = [3, 2 ** 63 - 1, -1]
    noise = SeededNoise(DEV).begin(seeds)
    for high in (10, 1000, 2 ** 31):          # label draws 0, 1, 2
        got = noise.randint(high)
        assert got.dtype == torch.int64 and got.tolist() == [sc.randint(s, noise.label_draw - 1, high) for s in seeds]
    first = noise.randn((3, 3, 8, 8))
    second = noise.randn_like(torch.empty(3, 5, dtype=torch.float64, device=DEV))
    assert first.dtype == torch.float32 and second.dtype == torch.float64 and (noise.draw, noise.label_draw) == (2, 3)
    assert torch.equal(first, ops.randn_seeded(noise.seeds, (3, 3, 8, 8), 0)) and torch.equal(second, ops.randn_seeded(noise.seeds, (3, 5), 1).double())
    address = noise.seeds.data_ptr()
    noise.begin(range(3))
    assert noise.seeds.data_ptr() == address and torch.equal(noise.randn((3, 4)), ops.randn_seeded(device_seeds([0, 1, 2]), (3, 4), 0))


# ---- the samplers --------------------------------------------------------------------------------------------------------
STEPS, SIZE, CLASSES, SEED, TOTAL = 4, 8, 10, 20240, 12
GENERATORS = ["ddim", "heun", "dpmpp2m_sde", "flow_sde"]
CAPTURABLE = GENERATORS[1:]


def ddim_chain(args):
    return vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(1000, str(STEPS)), args=args,
                                   betas=vaw_amd.get_named_beta_schedule("cosine", 1000), model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                   model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)


def make_sampler(name, **extra):
    st = dict(guidance_scale=1.8, sample_steps=STEPS)
    if name == "ddim":
        args = sampler_args("ddim", st, cpu_rng=False, **extra)
        diff = ddim_chain(args)
    elif name == "flow_sde":
        args = sampler_args("flow", dict(st, solver="heun", path_type="linear", mean_type="VELOCITY"), cpu_rng=False, sampler_type="sde", **extra)
        diff = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY)
    else:
        args = sampler_args("edm", dict(st, solver=name), cpu_rng=False, eta=0.8, **extra)
        diff = None
    return vaw_amd.Sampler(args, torch.device(DEV), Standin(sampling_model), diff)


def sample(name, num_samples, sample_size, manual_seed=None, **extra):
    """(float images, uint8 images, labels) of Sampler.sample, the batches concatenated."""
    s = make_sampler(name, **extra)
    floats, finish = [], s._inverse_normalize
    s._inverse_normalize = lambda x: (floats.append(x.detach().clone()), finish(x))[1]
    if manual_seed is not None:
        torch.manual_seed(manual_seed)
    images, labels = s.sample(num_samples, sample_size, SIZE, CLASSES)
    assert len(images) == len(labels) == len(floats) == -(-num_samples // sample_size)
    return torch.cat(floats).cpu(), np.concatenate(images), np.concatenate(labels)


@functools.lru_cache(maxsize=None)
def whole_set(name):
    """Global indices 0 .. 11 in one batch: what every other way of drawing them is compared with."""
    return sample(name, TOTAL, TOTAL, sample_seed=SEED)


def same(got, want, what):
    for g, w, part in zip(got, want, ("float images", "bytes", "labels")):
        g, w = (torch.as_tensor(v) for v in (g, w))
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {part} {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
        assert torch.equal(g, w), f"{what}: {int((g != w).sum())} {part} differ"


def part(triple, lo, hi):
    return tuple(v[lo:hi] for v in triple)


@pytest.mark.parametrize("name", GENERATORS)
def test_sampler_images_do_not_depend_on_the_batch_size(name):
    want = whole_set(name)
    assert want[0].shape == (TOTAL, 3, SIZE, SIZE) and want[1].shape == (TOTAL, SIZE, SIZE, 3) and want[2].shape == (TOTAL,)
    assert len({want[1][k].tobytes() for k in range(TOTAL)}) == TOTAL and len(set(want[2].tolist())) > 2
    assert want[2].tolist() == [sc.randint(SEED + k, 0, CLASSES) for k in range(TOTAL)]          # a label depends on k alone
    for sample_size in (2, 3, 4, 5):
        got = sample(name, TOTAL, sample_size, sample_seed=SEED)
        assert got[0].shape[0] == (15 if sample_size == 5 else TOTAL)
        same(part(got, 0, TOTAL), want, f"{name}, sample_size {sample_size}")


@pytest.mark.parametrize("name", GENERATORS)
def test_sampler_shards_and_restarts_reproduce_the_single_rank_set(name):
    want = whole_set(name)
    shards = [sample(name, 6, 3, sample_seed=SEED, sample_shard=(r, 2)) for r in (0, 1)]          # two batches of 3 on each rank
    order = [(r, n) for n in (0, 1) for r in (0, 1)]                                               # _gather_samples: batch-major
    got = tuple(np.concatenate([np.asarray(shards[r][i][3 * n:3 * n + 3]) for r, n in order]) for i in range(3))
    same(got, want, f"{name}, two shards interleaved")
    same(sample(name, 6, 3, sample_seed=SEED, sample_start=6), part(want, 6, TOTAL), f"{name}, sample_start 6")
    same(sample(name, 6, 2, sample_seed=SEED + 6), part(want, 6, TOTAL), f"{name}, seed S + 6 is start 6")


@pytest.mark.parametrize("name", CAPTURABLE)
def test_sampler_captured_graph_reproduces_the_eager_run(name):
    """Three batches of 4: eager, captured, replayed.  The seeds reach the replay through the SeededNoise's buffer."""
    want = whole_set(name)
    got = sample(name, TOTAL, 4, sample_seed=SEED, hip_graph=True)
    same(got, want, f"{name}, hip_graph")
    assert len({got[1][4 * b:4 * b + 4].tobytes() for b in range(3)}) == 3


@pytest.mark.parametrize("name", GENERATORS)
def test_another_sample_seed_changes_every_image(name):
    want, other = whole_set(name), sample(name, TOTAL, 4, sample_seed=SEED + 1000)
    assert all(want[1][k].tobytes() != other[1][k].tobytes() for k in range(TOTAL))
    same(part(sample(name, TOTAL, 4, sample_seed=SEED + 1), 0, TOTAL - 1), part(want, 1, TOTAL), f"{name}, seed S + 1 shifts the set by one")


def by_hand(name, s, labels):
    """One batch as Sampler draws it without args.sample_seed: the global generator, in the order labels (drawn by the caller),
    initial noise, then the solver's own draws."""
    a, n = s.args, labels.shape[0]
    latents = torch.randn([n, 3, SIZE, SIZE], device=DEV)
    if name == "ddim":
        return s.diffusion.ddim_sample_loop(s._build_cfg_model(CLASSES), (n, 3, SIZE, SIZE), noise=latents, device=DEV, model_kwargs={"y": labels})
    if name == "flow_sde":
        return vaw_amd.flow_sde_sample(s.diffusion, s._build_cfg_model(CLASSES), latents, DEV, num_steps=STEPS, solver="heun", y=labels)
    net = s._build_denoiser(SIZE, CLASSES)
    kw = dict(class_labels=labels, num_steps=STEPS, solver=name, discretization=a.discretization)
    if name == "heun":
        return vaw_amd.edm_sample(net, latents, schedule=a.schedule, scaling=a.scaling, **kw)
    return vaw_amd.dpm_sample(net, latents, eta=a.eta, **kw)


@pytest.mark.parametrize("name", GENERATORS)
def test_without_sample_seed_the_global_generator_is_drawn_as_before(name):
    got = sample(name, 6, 3, manual_seed=99)
    s = make_sampler(name)
    assert s._seed_plan() is None
    torch.manual_seed(99)
    for b in range(2):
        labels = torch.randint(0, CLASSES, (3,), device=DEV)
        x = by_hand(name, s, labels)
        same(part(got, 3 * b, 3 * b + 3), (x.cpu(), ops.finish_images(x).cpu().numpy(), labels.cpu().numpy()), f"{name}, batch {b}")
    assert s._noise is None


# ---- the loops called directly with a SeededNoise ----------------------------------------------------------------------------
def direct_edm(noise, labels, n, fused=None):
    net = vaw_amd.EDMDenoiser(Standin(sampling_model), SIZE, 3, label_dim=CLASSES, noise_schedule="cosine").to(DEV)
    return vaw_amd.edm_sample(net, noise.randn((n, 3, SIZE, SIZE)), labels, randn_like=noise.randn_like, num_steps=STEPS, S_churn=2.0, fused=fused)


def direct_dpm(noise, labels, n, fused=None):
    net = vaw_amd.EDMDenoiser(Standin(sampling_model), SIZE, 3, label_dim=CLASSES, noise_schedule="cosine").to(DEV)
    return vaw_amd.dpm_sample(net, noise.randn((n, 3, SIZE, SIZE)), labels, randn_like=noise.randn_like, num_steps=STEPS, solver="dpmpp2m_sde",
                              eta=0.8, fused=fused)


def direct_flow(noise, labels, n, fused=None):
    args = sampler_args("flow", dict(guidance_scale=1.0, path_type="linear"), cpu_rng=False)
    fm = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY)
    return vaw_amd.flow_sde_sample(fm, Standin(sampling_model), noise.randn((n, 3, SIZE, SIZE)), DEV, num_steps=STEPS, randn_like=noise.randn_like,
                                   fused=fused, y=labels)


def direct_p(noise, labels, n, fused=None):
    d = ddim_chain(sampler_args("ddim", dict(guidance_scale=1.0), cpu_rng=False))
    return d.p_sample_loop(Standin(sampling_model), (n, 3, SIZE, SIZE), device=DEV, model_kwargs={"y": labels}, randn_like=noise.randn_like)


def direct(fn, sample_size, fused=None, total=TOTAL, seed=SEED):
    noise, out, draws = SeededNoise(DEV), [], None
    for first in range(0, total, sample_size):
        noise.begin(range(seed + first, seed + first + sample_size))
        labels = noise.randint(CLASSES)
        out.append(fn(noise, labels, sample_size, fused))
        assert draws in (None, noise.draw)          # every batch walks the same trajectory
        draws = noise.draw
    return torch.cat(out)[:total], draws


@pytest.mark.parametrize("fn, draws", [(direct_edm, 1 + STEPS), (direct_dpm, STEPS), (direct_flow, STEPS), (direct_p, 1 + STEPS)],
                         ids=["edm_churn", "dpmpp2m_sde", "flow_sde", "p_sample_loop"])
def test_direct_loops_with_seeded_noise(fn, draws):
    """Draw 0 is the initial noise; then edm_sample draws every step, dpm_sample and flow_sde_sample every step but the last,
    p_sample_loop every step.  Bitwise the same image per seed at every batch size, fused and as the tensor composition."""
    want, n_draws = direct(fn, TOTAL)
    assert n_draws == draws and bool(torch.isfinite(want).all())
    for sample_size in (2, 3, 4, 5):
        got, _ = direct(fn, sample_size)
        assert torch.equal(got, want), f"sample_size {sample_size}: {int((got != want).sum())} elements differ"
    if fn is not direct_p:
        composed, n_draws = direct(fn, 4, fused=False)
        assert n_draws == draws and torch.equal(composed, want), f"fused=False: {int((composed != want).sum())} elements differ"
    other, _ = direct(fn, TOTAL, seed=SEED + 1000)
    assert all(not torch.equal(other[k], want[k]) for k in range(TOTAL))
    # the per-step draws matter: the same initial noise and labels under another stream of step noise give other images
    class Shifted(SeededNoise):
        def randn_like(self, x):
            return -super().randn_like(x)
    shifted = Shifted(DEV).begin(range(SEED, SEED + TOTAL))
    changed = fn(shifted, shifted.randint(CLASSES), TOTAL)
    assert all(not torch.equal(changed[k], want[k]) for k in range(TOTAL))

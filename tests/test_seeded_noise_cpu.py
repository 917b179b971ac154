"""Per-sample seeded noise without a GPU: the numpy restatement (tests/seeded_noise_cases.py) against the Random123 known-answer
vectors and against N(0, 1), and the host bookkeeping of vaw_amd.SeededNoise and of Sampler under args.sample_seed -- index
formula, draw counters, refusals.  No kernel is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import seeded_noise_cases as sc
from conftest import REPO, load_json, sampling_model
from sampler_cases import Standin, sampler_args, spaced

import abi_cases
import vaw_amd
from vaw_amd import _lib, ops
from vaw_amd.noise import SeededNoise

N_STAT = 1 << 20


def test_restatement_reproduces_the_random123_known_answers():
    vectors = load_json("philox_kat.json")["vectors"]
    assert len(vectors) == 3
    for v in vectors:
        got = sc.philox4x32_10([int(w, 16) for w in v["counter"]], [int(w, 16) for w in v["key"]])
        assert [f"{int(w):08x}" for w in got] == v["result"]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 2 ** 63 - 1, -1])
def test_restatement_normals_are_standard_normal(seed):
    """2^20 normals of draw 0: mean, variance and excess kurtosis within 4 standard errors (1/sqrt N, sqrt(2/N), sqrt(24/N)) of
    0, 1, 0, and the Kolmogorov-Smirnov p-value against N(0, 1) above 1e-3."""
    z = sc.normal(seed, 0, N_STAT)
    mean, var = float(z.mean()), float(z.var())
    kurt = float(((z - mean) ** 4).mean()) / var ** 2 - 3.0
    p = sc.ks_pvalue(z)
    print(f"seed {seed}: mean {mean * math.sqrt(N_STAT):+.2f} se, variance {(var - 1) / math.sqrt(2 / N_STAT):+.2f} se, "
          f"excess kurtosis {kurt / math.sqrt(24 / N_STAT):+.2f} se, KS p = {p:.3f}")
    assert abs(mean) <= 4 / math.sqrt(N_STAT)
    assert abs(var - 1) <= 4 * math.sqrt(2 / N_STAT)
    assert abs(kurt) <= 4 * math.sqrt(24 / N_STAT)
    assert p > 1e-3


def test_restatement_streams_are_uncorrelated_across_seeds_and_draws():
    a = sc.normal(5, 0, N_STAT)
    for what, b in (("seeds 5 and 6", sc.normal(6, 0, N_STAT)), ("draws 0 and 1 of seed 5", sc.normal(5, 1, N_STAT))):
        r = float(np.corrcoef(a, b)[0, 1])
        print(f"{what}: correlation {r * math.sqrt(N_STAT):+.2f} / sqrt N")
        assert abs(r) <= 4 / math.sqrt(N_STAT)


def test_restatement_prefix_property_and_uniform_range():
    for fn in (sc.bits, sc.uniform, sc.normal):
        assert np.array_equal(fn(3, 2, 8)[:5], fn(3, 2, 5))
    assert sc.uniform_of(np.array([0, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [2.0 ** -33, 1.0]
    assert not np.array_equal(sc.bits(3, 2, 8), sc.bits(3, 2, 8, sc.TAG_LABELS))


# ---- the C entry point: declared, bound, exported, and refusing before any launch --------------------------------------
def test_randn_seeded_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    lib = vaw_amd.lib()
    assert re.search(r"\bint vaw_randn_seeded\(", header) and "vaw_randn_seeded" in vaw_amd.exported_symbols() and hasattr(lib, "vaw_randn_seeded")
    assert len(abi_cases.assert_bound_as_declared(lib, "vaw_randn_seeded")) == 9
    for name, value in (("VAW_NOISE_BITS", ops.NOISE_MODES["bits"]), ("VAW_NOISE_UNIFORM", ops.NOISE_MODES["uniform"]),
                        ("VAW_NOISE_NORMAL", ops.NOISE_MODES["normal"]), ("VAW_NOISE_TAG_NOISE", ops.NOISE_TAG_NOISE),
                        ("VAW_NOISE_TAG_LABELS", ops.NOISE_TAG_LABELS)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert re.search(r"\bVAW_F64 = 4\b", header) and _lib.F64 == 4


def test_randn_seeded_refuses_bad_arguments_before_any_launch():
    lib = vaw_amd.lib()
    buf = (ctypes.c_double * 8)()          # host memory: a call that did launch would fail on it, none does
    addr = ctypes.addressof(buf)
    for call, word in sc.refused_calls(addr, addr):
        assert lib.vaw_randn_seeded(*call, None) == -1 and word in lib.vaw_last_error_string().decode(), (call, word)


def test_no_cpu_fallback():
    seeds = torch.arange(3)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.randn_seeded(seeds, (3, 4), 0)
    with pytest.raises(vaw_amd.VawError, match="GPU only"):
        ops.randn_seeded(seeds, torch.zeros(3, 4), 0)
    noise = SeededNoise("cpu").begin(range(3))
    for draw in (lambda: noise.randn((3, 4)), lambda: noise.randn_like(torch.zeros(3, 4)), lambda: noise.randint(10)):
        with pytest.raises(vaw_amd.VawError, match="GPU only"):
            draw()
    assert (noise.draw, noise.label_draw) == (0, 0)          # a refused draw does not move the counters


# ---- SeededNoise: host bookkeeping (the kernel call replaced by a recorder) -------------------------------------------------
class Recorder:
    def __init__(self, word=0):
        self.calls, self.word = [], word

    def __call__(self, seeds, shape_or_like, draw, *, tag=0, mode="normal", dtype=None, out=None):
        like = shape_or_like if torch.is_tensor(shape_or_like) else None
        shape = tuple(like.shape) if like is not None else tuple(shape_or_like)
        self.calls.append((seeds.tolist(), shape, draw, tag, mode, dtype if dtype is not None else (like.dtype if like is not None else None)))
        if mode == "bits":
            return torch.full(shape, self.word, dtype=torch.int32)
        return torch.zeros(shape, dtype=self.calls[-1][5] or torch.float32)


def test_seeded_noise_counts_draws_and_begin_resets_them(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(vaw_amd.noise.ops, "randn_seeded", rec)
    noise = SeededNoise("cpu")
    with pytest.raises(RuntimeError, match="begin"):
        noise.randn((2, 3))
    assert noise.begin([7, 8]) is noise
    address = noise.seeds.data_ptr()
    assert noise.randn((2, 3, 4)).dtype == torch.float32
    assert noise.randn_like(torch.zeros(2, 5, dtype=torch.float64)).dtype == torch.float64
    assert noise.randint(10).shape == (2,) and noise.randint(10).dtype == torch.int64
    noise.randn([2, 1])
    assert [(c[2], c[3], c[4]) for c in rec.calls] == [(0, 0, "normal"), (1, 0, "normal"), (0, 1, "bits"), (1, 1, "bits"), (2, 0, "normal")]
    assert all(c[0] == [7, 8] for c in rec.calls) and rec.calls[2][1] == (2, 1)
    assert (noise.draw, noise.label_draw) == (3, 2)
    noise.begin(torch.tensor([-1, 2 ** 63 - 1]))
    assert noise.seeds.data_ptr() == address and noise.seeds.tolist() == [-1, 2 ** 63 - 1]          # same B: the same buffer
    assert (noise.draw, noise.label_draw) == (0, 0)
    noise.randn((2, 2))
    assert rec.calls[-1][:3] == ([-1, 2 ** 63 - 1], (2, 2), 0)
    noise.begin(range(5, 8))
    assert noise.seeds.tolist() == [5, 6, 7]


def test_seeded_noise_refusals(monkeypatch):
    monkeypatch.setattr(vaw_amd.noise.ops, "randn_seeded", Recorder())
    noise = SeededNoise("cpu").begin([1, 2, 3])
    for bad in ((2, 4), (4,), ()):
        with pytest.raises(ValueError, match="leading dimension"):
            noise.randn(bad)
    with pytest.raises(ValueError, match="leading dimension"):
        noise.randn_like(torch.zeros(4, 3))
    for high in (0, -1, 2 ** 31 + 1):
        with pytest.raises(ValueError, match="high"):
            noise.randint(high)
    assert (noise.draw, noise.label_draw) == (0, 0)
    for seeds in ([2 ** 63], [-2 ** 63 - 1], [], torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            noise.begin(seeds)


@pytest.mark.parametrize("high", [1, 10, 1000, 2 ** 31])
def test_seeded_noise_randint_scales_the_word(monkeypatch, high):
    for word in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, int(sc.bits(11, 0, 1, sc.TAG_LABELS)[0])):
        signed = word - (1 << 32) if word >= 1 << 31 else word          # the int32 that holds the word
        monkeypatch.setattr(vaw_amd.noise.ops, "randn_seeded", Recorder(signed))
        got = SeededNoise("cpu").begin([11, 12]).randint(high)
        assert got.tolist() == [(word * high) >> 32] * 2 and 0 <= int(got[0]) < high
    assert sc.randint(11, 0, high) == (int(sc.bits(11, 0, 1, sc.TAG_LABELS)[0]) * high) >> 32


# ---- Sampler under args.sample_seed: the index formula and the refusals ----------------------------------------------------
def seeded_sampler(**kw):
    args = sampler_args("ddim", dict(guidance_scale=1.0), **{"cpu_rng": False, **kw})
    return vaw_amd.Sampler(args, torch.device("cpu"), Standin(sampling_model), None)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("start", [0, 6])
def test_sampler_index_formula_partitions_the_range(world, start):
    sample_size, n_batches, S = 4, 3, 1000
    seen = []
    for rank in range(world):
        s = seeded_sampler(sample_seed=S, sample_start=start, **({"sample_shard": (rank, world)} if world > 1 else {}))
        assert s._seed_plan() == (S, start, rank, world)
        for n in range(n_batches):
            idx = list(s._sample_indices(n, sample_size))
            assert idx == sc.sample_indices(start, world, rank, n, sample_size)
            assert idx[0] == start + (n * world + rank) * sample_size and idx == list(range(idx[0], idx[0] + sample_size))
            assert s._sample_seeds(n, sample_size) == [S + k for k in idx]
            seen.append((n, rank, idx))
    seen.sort()          # batch-major, rank-minor: the order _gather_samples lays the gathered batches out in
    assert [k for _, _, idx in seen for k in idx] == list(range(start, start + n_batches * world * sample_size))


def test_sampler_seeds_wrap_as_64_bit_patterns():
    s = seeded_sampler(sample_seed=2 ** 63 - 2)
    assert s._sample_seeds(0, 4) == [2 ** 63 - 2, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 1]
    assert [sc.key_of(v) for v in s._sample_seeds(0, 4)] == [sc.key_of(2 ** 63 - 2 + k) for k in range(4)]


def test_sampler_without_sample_seed_has_no_plan():
    s = seeded_sampler()
    assert s._seed_plan() is None and s._noise is None
    assert vaw_amd.SeededNoise is SeededNoise          # re-exported


@pytest.mark.parametrize("kw, word", [
    (dict(sample_seed=1, cpu_rng=True), "cpu_rng"),
    (dict(sample_seed=1, sample_shard=(0, 2), parallel=True), "parallel"),
    (dict(sample_seed=-1), "sample_seed"), (dict(sample_seed=2 ** 63), "sample_seed"), (dict(sample_seed=1.5), "sample_seed"),
    (dict(sample_seed=True), "sample_seed"),
    (dict(sample_seed=1, sample_start=-1), "sample_start"), (dict(sample_seed=1, sample_start=0.5), "sample_start"),
    (dict(sample_seed=1, sample_shard=(2, 2)), "sample_shard"), (dict(sample_seed=1, sample_shard=(-1, 2)), "sample_shard"),
    (dict(sample_seed=1, sample_shard=3), "sample_shard"),
    (dict(sample_shard=(0, 2)), "sample_seed"), (dict(sample_start=3), "sample_seed"),
])
def test_sampler_refusals(kw, word):
    s = seeded_sampler(**kw)
    with pytest.raises(ValueError, match=word):
        s.sample(3, 3, 8, 10)


def test_sample_loops_refuse_a_hook_together_with_cpu_rng():
    args = sampler_args("ddim", dict(guidance_scale=1.0))
    assert args.cpu_rng
    d, model = spaced("ddim25_eps_fixed", args)
    hook = lambda x: torch.zeros_like(x)
    for loop in (d.p_sample_loop, d.ddim_sample_loop):
        with pytest.raises(ValueError, match="cpu_rng"):
            loop(model, (2, 3, 8, 8), device="cpu", randn_like=hook)
    for loop in (d.p_sample_loop_progressive, d.ddim_sample_loop_progressive):
        with pytest.raises(ValueError, match="cpu_rng"):
            next(loop(model, (2, 3, 8, 8), device="cpu", randn_like=hook))

"""Shared by test_seeded_noise_cpu.py and test_gpu_seeded_noise.py: a numpy restatement of the per-sample seeded noise
(vaw_randn_seeded, vaw_amd.SeededNoise, Sampler under args.sample_seed), written from the published definition of
Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known-answer
vectors are in tests/golden/philox_kat.json) and from the layout the package documents, not from its code:

  block c of sample b   = philox4x32_10(counter (c, draw, tag, 0), key (seed & 0xffffffff, seed >> 32 as unsigned 64 bits))
  elements 4c .. 4c+3   = its four words
  uniform               = float32(float64(float32(r)) * 2^-32 + 2^-33): the product and the sum are exact in float64, so the one
                          rounding to float32 is the rounding of the fused multiply-add
  normals               = Box-Muller: words (r0, r1) -> sqrt(-2 log u0) * (cos, sin)(2 pi u1), words (r2, r3) -> the next two
  label                 = (r * high) >> 32 of word 0 of block 0 under tag 1
  global index          = start + (batch * world + rank) * sample_size + row"""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TAG_NOISE, TAG_LABELS = 0, 1
F32, BF16, FP8, F64 = 0, 1, 2, 4          # vaw_dtype of include/vaw_hip.h


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) of 32-bit values; key: two.  Returns the four output words, uint64 arrays."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) for v in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 bits: exact in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
    return c


def key_of(seed):
    s = int(seed) % (1 << 64)          # the int64 read as an unsigned 64-bit pattern
    return s & 0xFFFFFFFF, s >> 32


def bits(seed, draw, n, tag=TAG_NOISE):
    """The first n words of draw `draw` of the stream `seed`: uint32 [n]."""
    blocks = (n + 3) // 4
    z = np.zeros(blocks, dtype=np.uint64)
    words = philox4x32_10((np.arange(blocks, dtype=np.uint64), z + np.uint64(draw), z + np.uint64(tag), z), key_of(seed))
    return np.stack(words, axis=1).reshape(-1)[:n].astype(np.uint32)


def uniform_of(words):
    r = words.astype(np.float32).astype(np.float64)
    return (r * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def uniform(seed, draw, n, tag=TAG_NOISE):
    return uniform_of(bits(seed, draw, n, tag))


def _box_muller(u, dtype):
    """u: float32 uniforms, a multiple of 4 of them.  Box-Muller evaluated in `dtype`."""
    u = u.astype(dtype).reshape(-1, 2, 2)
    rad = np.sqrt(dtype(-2.0) * np.log(u[:, :, 0]))
    ang = dtype(2.0 * math.pi) * u[:, :, 1]
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(-1)


def normal(seed, draw, n, dtype=np.float64):
    """float64 (the reference) or float32 (the yardstick of what float32 arithmetic costs) normals: [n]."""
    return _box_muller(uniform(seed, draw, 4 * ((n + 3) // 4)), dtype)[:n]


def randint(seed, draw, high):
    return (int(bits(seed, draw, 1, TAG_LABELS)[0]) * int(high)) >> 32


def sample_indices(start, world, rank, batch, sample_size):
    first = start + (batch * world + rank) * sample_size
    return list(range(first, first + sample_size))


def ks_pvalue(x):
    """Two-sided Kolmogorov-Smirnov test of x against N(0, 1): the asymptotic Kolmogorov distribution with Stephens' finite-n
    correction (sqrt(n) + 0.12 + 0.11 / sqrt(n)) D."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    return min(1.0, max(0.0, 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))))


def refused_calls(out, seeds):
    """Every call vaw_randn_seeded must refuse, as (argument tuple, word of the message).  out / seeds: valid addresses."""
    ok = dict(out=out, dtype=F32, seeds=seeds, B=2, per_sample=8, draw=0, tag=0, mode=2)
    cases = [(dict(out=None), "null"), (dict(seeds=None), "null"), (dict(B=0), "sizes"), (dict(per_sample=0), "sizes"),
             (dict(per_sample=1 << 34), "2^34"), (dict(draw=-1), "draw"), (dict(draw=1 << 32), "draw"), (dict(tag=-1), "tag"),
             (dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(dtype=FP8), "dtype"), (dict(dtype=7), "dtype"),
             (dict(mode=0, dtype=BF16), "4 bytes"), (dict(mode=1, dtype=F64), "4 bytes"), (dict(mode=0, dtype=F64), "4 bytes"),
             (dict(out=out + 2), "aligned"), (dict(dtype=F64, out=out + 4), "aligned")]
    order = ("out", "dtype", "seeds", "B", "per_sample", "draw", "tag", "mode")
    return [(tuple({**ok, **c}[k] for k in order), word) for c, word in cases]

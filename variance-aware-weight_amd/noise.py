"""Per-sample seeded noise for the samplers: the role of `StackedRandomGenerator` in EDM's generate.py, as one counter-based
kernel (vaw_randn_seeded, csrc/noise.hip).  Row b of every draw is a pure function of (seeds[b], draw number, element), so the
image of a seed does not depend on the batch it is drawn in, on the rank that draws it, or on whether the loop runs eagerly
or as a captured graph."""
import torch

from . import ops

__all__ = ["SeededNoise"]

SEED_MIN, SEED_MAX = -2 ** 63, 2 ** 63 - 1


class SeededNoise:
    """`begin(seeds)` starts the trajectories of a batch of B samples; `randn(shape)` / `randn_like(x)` are draw number 0, 1, 2, ...
    of those B streams (leading dimension B), `randint(high)` draws labels from a stream of its own (tag 1) with its own counter.

    The draw counters are host integers: a launch made inside a graph capture has its draw number baked in, which is what a
    replay wants -- it walks the same trajectory again, on the seeds that are in the buffer then.  The buffer keeps its address
    while B does not change, so `begin` before a replay is all it takes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.seeds = None          # int64 [B] on the device
        self.draw = 0              # the next draw number of randn / randn_like
        self.label_draw = 0        # the next draw number of randint

    def begin(self, seeds):
        """seeds: an int64 tensor, a list or a range of length B >= 1, each in [-2^63, 2^63) (read as a 64-bit pattern)."""
        if torch.is_tensor(seeds):
            if seeds.dtype != torch.int64 or seeds.dim() != 1:
                raise ValueError(f"SeededNoise.begin: seeds must be a one-dimensional int64 tensor, got {seeds.dtype} {tuple(seeds.shape)}")
            src = seeds
        else:
            values = [int(s) for s in seeds]
            bad = [s for s in values if not SEED_MIN <= s <= SEED_MAX]
            if bad:
                raise ValueError(f"SeededNoise.begin: seed {bad[0]} outside [-2^63, 2^63)")
            src = torch.tensor(values, dtype=torch.int64)
        if src.numel() < 1:
            raise ValueError("SeededNoise.begin: no seeds")
        if self.seeds is None or self.seeds.shape != src.shape:
            self.seeds = torch.empty(src.shape, dtype=torch.int64, device=self.device)
        self.seeds.copy_(src)
        self.draw = self.label_draw = 0
        return self

    def _batch(self, what, lead=None):
        if self.seeds is None:
            raise RuntimeError(f"SeededNoise.{what}: call begin(seeds) first")
        B = self.seeds.shape[0]
        if lead is not None and lead != B:
            raise ValueError(f"SeededNoise.{what}: leading dimension {lead} is not the {B} seeds of begin()")
        return B

    def randn(self, shape, dtype=torch.float32):
        shape = tuple(int(s) for s in shape)
        self._batch("randn", shape[0] if shape else 0)
        out = ops.randn_seeded(self.seeds, shape, self.draw, dtype=dtype)
        self.draw += 1
        return out

    def randn_like(self, x):
        self._batch("randn_like", x.shape[0] if x.dim() else 0)
        out = ops.randn_seeded(self.seeds, x, self.draw)
        self.draw += 1
        return out

    def randint(self, high):
        """int64 [B] in [0, high): the first word of the label stream, scaled as (r * high) >> 32.  high in [1, 2^31]."""
        high = int(high)
        if not 1 <= high <= 2 ** 31:
            raise ValueError(f"SeededNoise.randint: high {high} outside [1, 2^31]")
        B = self._batch("randint")
        bits = ops.randn_seeded(self.seeds, (B, 1), self.label_draw, tag=ops.NOISE_TAG_LABELS, mode="bits")
        self.label_draw += 1
        return ((bits.view(B).to(torch.int64) & 0xFFFFFFFF) * high) >> 32

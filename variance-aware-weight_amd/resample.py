"""Timestep importance samplers, same API as the reference's tools/resample.py (which nothing in the
reference calls: `Trainer` draws t through GaussianDiffusion.sample_t).  Host-side float64 numpy by nature:
T=1000 weights and a [T,10] loss history; the only device traffic is the batch of indices/weights going up
and, for the loss-aware sampler, one all_gather of (t, loss) pairs per step."""
from abc import ABC, abstractmethod

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L


class ScheduleSampler(ABC):
    @abstractmethod
    def weights(self):
        """numpy array [T] of positive (unnormalised) weights."""

    def sample(self, batch_size, device):
        w = self.weights()
        p = w / np.sum(w)
        indices_np = np.random.choice(len(p), size=(batch_size,), p=p)
        indices = torch.from_numpy(indices_np).long().to(device)
        weights = torch.from_numpy(1 / (len(p) * p[indices_np])).float().to(device)
        return indices, weights


class UniformSampler(ScheduleSampler):
    def __init__(self, diffusion):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])

    def weights(self):
        return self._weights


class LossAwareSampler(ScheduleSampler):
    def update_with_local_losses(self, local_ts, local_losses):
        """Every rank contributes its (t, loss) pairs; all ranks end with identical history.
        One padded all_gather of a [max_bs, 2] float64 tensor (the reference issues three collectives)."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            world = dist.get_world_size()
            n = torch.tensor([len(local_ts)], dtype=torch.int64, device=local_ts.device)
            sizes = [torch.zeros_like(n) for _ in range(world)]
            dist.all_gather(sizes, n)
            sizes = [int(s.item()) for s in sizes]
            mx = max(sizes)
            pack = torch.zeros(mx, 2, dtype=torch.float64, device=local_ts.device)
            pack[: len(local_ts), 0] = local_ts.double()
            pack[: len(local_ts), 1] = local_losses.double()
            out = [torch.zeros_like(pack) for _ in range(world)]
            dist.all_gather(out, pack)
            timesteps = [int(v) for o, s in zip(out, sizes) for v in o[:s, 0].tolist()]
            losses = [float(v) for o, s in zip(out, sizes) for v in o[:s, 1].tolist()]
        else:
            timesteps, losses = local_ts.tolist(), local_losses.tolist()
        self.update_with_all_losses(timesteps, losses)

    @abstractmethod
    def update_with_all_losses(self, ts, losses):
        ...


class LossSecondMomentResampler(LossAwareSampler):
    """w_t = sqrt(mean of the last `history_per_term` squared losses seen at t), mixed with a uniform floor once
    every timestep has a full history.  The history is a ring per timestep: the weight is a mean of squares,
    so it does not depend on the order in which the last 10 losses are stored."""

    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        self.diffusion = diffusion
        self.history_per_term = history_per_term
        self.uniform_prob = uniform_prob
        T = diffusion.num_timesteps
        self._ring = np.zeros((T, history_per_term), dtype=np.float64)
        self._seen = np.zeros(T, dtype=np.int64)      # total losses ever recorded per timestep

    @property
    def _loss_counts(self):
        return np.minimum(self._seen, self.history_per_term)

    def _warmed_up(self):
        return bool((self._seen >= self.history_per_term).all())

    def weights(self):
        T = self.diffusion.num_timesteps
        if not self._warmed_up():
            return np.ones(T, dtype=np.float64)
        w = np.sqrt((self._ring ** 2).mean(axis=-1))
        w = w / w.sum() * (1 - self.uniform_prob)
        return w + self.uniform_prob / T

    def update_with_all_losses(self, ts, losses):
        H = self.history_per_term
        for t, loss in zip(ts, losses):
            self._ring[t, self._seen[t] % H] = loss
            self._seen[t] += 1


class DeviceLossSecondMomentResampler(ScheduleSampler):
    """LossSecondMomentResampler with its state in device memory: `ring` f64 [T, H] and `seen` i64 [T] sit next to the
    diffusion tables, vaw_resampler_draw draws t and the 1/(T p_t) weights from them and vaw_resampler_update records the
    per-sample losses.  Neither `sample` nor the updates touch the host, so a step stays free of host synchronisation and
    can be captured into a hipGraph (every buffer the kernels write is allocated here, once).  Same arithmetic as the host
    class in the same f64; the sums run in the fixed orders include/vaw_hip.h states, so p agrees with the host's to a few
    roundings, not bitwise.  GPU only: there is no CPU fallback."""

    def __init__(self, diffusion, device, history_per_term=10, uniform_prob=0.001):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise L.VawError(f"DeviceLossSecondMomentResampler keeps its history on the GPU: got device '{device}' (no CPU fallback "
                             "exists by design; the host sampler is \"loss-second-moment\")")
        self.diffusion, self.device = diffusion, device
        self.history_per_term, self.uniform_prob = int(history_per_term), float(uniform_prob)
        # parity runs draw the uniforms from numpy's global stream, the one np.random.choice consumes in the host sampler
        self.cpu_rng = bool(getattr(getattr(diffusion, "args", None), "cpu_rng", False))
        T = self.num_timesteps = int(diffusion.num_timesteps)
        self.ring = torch.zeros(T, self.history_per_term, dtype=torch.float64, device=device)
        self.seen = torch.zeros(T, dtype=torch.int64, device=device)
        self._p = torch.zeros(T, dtype=torch.float64, device=device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)
        # runs behind the step guard (Trainer, args.skip_nonfinite): pairs whose loss is inf or NaN are not recorded but counted
        # (vaw_resampler_update_finite), so a refused step leaves no trace in the history either
        self.skip_nonfinite = False

    def sample(self, batch_size, device=None):
        """(indices i64 [B], weights f32 [B]) on the sampler's device; enqueues one kernel, never synchronises."""
        if device is not None and torch.device(device).type != "cuda":
            raise L.VawError(f"DeviceLossSecondMomentResampler.sample: device '{device}' is not the GPU the history lives on")
        B = int(batch_size)
        if self.cpu_rng:
            u = torch.from_numpy(np.random.random_sample(B)).to(self.device)
        else:
            u = torch.rand(B, dtype=torch.float64, device=self.device)
        return self._draw(u)

    def _draw(self, u):
        L.need_cuda(u)
        assert u.dtype == torch.float64 and u.dim() == 1 and u.is_contiguous()
        B = u.numel()
        idx = torch.empty(B, dtype=torch.int64, device=self.device)
        w = torch.empty(B, dtype=torch.float32, device=self.device)
        L.check(L.lib().vaw_resampler_draw(L.ptr(self.ring), L.ptr(self.seen), self.num_timesteps, self.history_per_term,
                                           self.uniform_prob, L.ptr(u), B, L.ptr(idx), L.ptr(w), L.ptr(self._p), L.stream_ptr()),
                "vaw_resampler_draw")
        return idx, w

    def update_with_all_losses(self, ts, losses):
        """Record the (t, loss) pairs in order; device tensors (anything else is copied up first)."""
        ts = torch.as_tensor(ts, device=self.device).to(torch.int64).contiguous()
        losses = torch.as_tensor(losses, device=self.device).to(torch.float32).contiguous()
        if ts.shape != losses.shape or ts.dim() != 1:
            raise L.VawError(f"update_with_all_losses: ts {tuple(ts.shape)} and losses {tuple(losses.shape)} must be equal 1-d shapes")
        name = "vaw_resampler_update_finite" if self.skip_nonfinite else "vaw_resampler_update"
        L.check(getattr(L.lib(), name)(L.ptr(ts), L.ptr(losses), ts.numel(), self.num_timesteps, self.history_per_term,
                                       L.ptr(self.ring), L.ptr(self.seen), L.ptr(self._bad), L.stream_ptr()), name)

    def update_with_local_losses(self, local_ts, local_losses):
        """World 1: the update kernel on the given tensors.  World > 1: ONE all_gather_into_tensor of a fixed [n, 2] f64 pack
        (an f32 loss and a timestep are both exact in f64), then one update over the world * n pairs in rank-major order, so
        every rank ends with the same history.  Every rank must pass the same local batch size n: that is NOT checked, because
        a check across ranks would be a host synchronisation -- ragged batches keep the host sampler."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            n = local_ts.numel()
            pack = torch.stack([local_ts.to(torch.float64), local_losses.detach().to(torch.float64)], dim=1).contiguous()
            out = torch.empty(dist.get_world_size() * n, 2, dtype=torch.float64, device=pack.device)
            dist.all_gather_into_tensor(out, pack)
            local_ts, local_losses = out[:, 0].to(torch.int64), out[:, 1].to(torch.float32)
        self.update_with_all_losses(local_ts, local_losses)

    def weights(self):
        """numpy f64 [T]: the p the kernel forms from the current history (1/T until every timestep has a full history; the
        host class returns ones there, the same distribution unnormalised).  Synchronises: for inspection, not for the step."""
        self._draw(torch.empty(0, dtype=torch.float64, device=self.device))
        return self._p.cpu().numpy()

    def invalid_count(self):
        """(t, loss) pairs skipped so far because t was outside [0, T) (or, with skip_nonfinite, the loss not finite).  Synchronises."""
        return int(self._bad.item())

    def state_dict(self):
        return {"ring": self.ring.detach().cpu().clone(), "seen": self.seen.detach().cpu().clone()}

    def load_state_dict(self, sd):
        ring, seen = torch.as_tensor(sd["ring"]), torch.as_tensor(sd["seen"])
        if tuple(ring.shape) != tuple(self.ring.shape) or tuple(seen.shape) != tuple(self.seen.shape):
            raise L.VawError(f"load_state_dict: history {tuple(ring.shape)} / {tuple(seen.shape)} does not fit a sampler of "
                             f"{tuple(self.ring.shape)} / {tuple(self.seen.shape)}")
        self.ring.copy_(ring.to(torch.float64))          # in place: a captured step keeps the addresses
        self.seen.copy_(seen.to(torch.int64))

    @classmethod
    def from_host(cls, sampler, device):
        """A device sampler that continues a LossSecondMomentResampler's history."""
        new = cls(sampler.diffusion, device, sampler.history_per_term, sampler.uniform_prob)
        new.load_state_dict(host_state_dict(sampler))
        return new

    def to_host(self):
        """A LossSecondMomentResampler that continues this history."""
        return host_from_state_dict(self.diffusion, self.state_dict(), self.history_per_term, self.uniform_prob)


def host_state_dict(sampler):
    """The state of a LossSecondMomentResampler in the device sampler's checkpoint format."""
    return {"ring": torch.from_numpy(sampler._ring.copy()), "seen": torch.from_numpy(sampler._seen.copy())}


def host_from_state_dict(diffusion, sd, history_per_term=10, uniform_prob=0.001):
    host = LossSecondMomentResampler(diffusion, history_per_term, uniform_prob)
    ring, seen = torch.as_tensor(sd["ring"]).numpy(), torch.as_tensor(sd["seen"]).numpy()
    if ring.shape != host._ring.shape or seen.shape != host._seen.shape:
        raise ValueError(f"history {ring.shape} / {seen.shape} does not fit a sampler of {host._ring.shape} / {host._seen.shape}")
    host._ring[...] = ring
    host._seen[...] = seen
    return host


def create_named_schedule_sampler(name, diffusion, device=None):
    """`device` places the state of "loss-second-moment-device"; the host samplers ignore it."""
    if name == "uniform":
        return UniformSampler(diffusion)
    if name == "loss-second-moment":
        return LossSecondMomentResampler(diffusion)
    if name == "loss-second-moment-device":
        return DeviceLossSecondMomentResampler(diffusion, device)
    raise NotImplementedError(f"unknown schedule sampler: {name}")

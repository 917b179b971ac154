"""Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3).

During training `PowerEMA` tracks up to four power-function averages of the model's flat f32 parameter buffer, two launches a step
with no host value in them (csrc/ema.hip), and writes snapshots of them.  Afterwards `posthoc_ema` synthesises the average of ANY
relative width at any snapshot time as the least-squares combination of the stored snapshots, folded in float64 on the device.

  profile      sigma_rel -> gamma > -1 with sigma_rel^2 = (gamma + 1) / ((gamma + 2)^2 (gamma + 3)); the average that ends at time t
               weighs the past with p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t]
  tracking     update t = 1, 2, ...:  e <- e + (p - e) c_t,  c_t = 1 - (1 - 1/t)^(gamma + 1)   (c_1 = 1: an exact copy)
  inner product  <a, b> = (ga + 1)(gb + 1) (ta / tb)^gb / ((ga + gb + 1) tb)  for ta <= tb
  coefficients   A x = b with A_ij = <i, j>, b_i = <i, out>, then x / sum(x); snapshots later than the target take no part

The host mathematics is float64 numpy; the tensors never leave the HIP path (no CPU fallback for them)."""
import math
import operator
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .flat import FlatModule

SIGMA_REL_MAX = 0.28          # the formula peaks at 1 / sqrt(12) = 0.2887 as gamma -> -1; beyond 0.28 gamma < -0.92 and c_t explodes
SNAPSHOT_FORMAT = "vaw_amd.power_ema.v1"


class NotFlatModuleError(TypeError, ValueError):
    """The model is not a FlatModule: a TypeError, as FusedAdamW raises for the same mistake, and a ValueError, as every other
    refusal of this module is."""


# ---- host mathematics -------------------------------------------------------------------------------------------------------------
def _check_sigma_rel(s):
    try:
        v = float(s)
    except (TypeError, ValueError):
        raise ValueError(f"sigma_rel {s!r} is not a number") from None
    if not (0.0 < v <= SIGMA_REL_MAX):
        raise ValueError(f"sigma_rel {s!r} is outside (0, {SIGMA_REL_MAX}]")
    return v


def _check_step(t, what="step"):
    if isinstance(t, bool):
        raise ValueError(f"{what} {t!r} is not a positive integer")
    try:
        v = operator.index(t)
    except TypeError:
        raise ValueError(f"{what} {t!r} is not a positive integer") from None
    if v < 1:
        raise ValueError(f"{what} {t!r} is not a positive integer")
    return v


def gamma_to_sigma_rel(gamma):
    g = float(gamma)
    if not g > -1.0:
        raise ValueError(f"gamma {gamma!r} must be larger than -1")
    return math.sqrt((g + 1.0) / ((g + 2.0) ** 2 * (g + 3.0)))


def sigma_rel_to_gamma(sigma_rel):
    """The largest real root of g^3 + 7 g^2 + (16 - s) g + (12 - s) = 0, s = sigma_rel^-2, polished by Newton steps on the cubic."""
    s = _check_sigma_rel(sigma_rel) ** -2
    roots = np.roots([1.0, 7.0, 16.0 - s, 12.0 - s])
    g = float(max(r.real for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real))))
    for _ in range(3):
        f = ((g + 7.0) * g + (16.0 - s)) * g + (12.0 - s)
        g -= f / ((3.0 * g + 14.0) * g + (16.0 - s))
    return g


def power_ema_coefficient(t, gamma):
    """c_t = 1 - (1 - 1/t)^(gamma + 1) in float64, as -expm1((gamma + 1) log1p(-1/t)): no cancellation at large t."""
    t, g = _check_step(t, "t"), float(gamma)
    if not g > -1.0:
        raise ValueError(f"gamma {gamma!r} must be larger than -1")
    return 1.0 if t == 1 else -math.expm1((g + 1.0) * math.log1p(-1.0 / t))


def profile_dot(t_a, gamma_a, t_b, gamma_b):
    """<p_{ta,ga}, p_{tb,gb}> of the continuous profiles; symmetric."""
    ta, ga, tb, gb = float(t_a), float(gamma_a), float(t_b), float(gamma_b)
    if ta > tb:
        ta, ga, tb, gb = tb, gb, ta, ga
    return (ga + 1.0) * (gb + 1.0) * (ta / tb) ** gb / ((ga + gb + 1.0) * tb)


def posthoc_coefficients(in_steps, in_sigma_rels, out_step, out_sigma_rel):
    """float64 [n]: the weights of the n stored averages (in_steps[i], in_sigma_rels[i]) whose sum best matches, in the least-squares
    sense over the profiles, the average of width out_sigma_rel ending at out_step.  They sum to 1; entries later than out_step
    are 0.  ValueError: a bad width or step, a duplicate (step, sigma_rel) pair, nothing at or before out_step."""
    steps = [_check_step(t) for t in in_steps]
    rels = [_check_sigma_rel(s) for s in in_sigma_rels]
    t_out, s_out = _check_step(out_step, "out_step"), _check_sigma_rel(out_sigma_rel)
    if len(steps) != len(rels):
        raise ValueError(f"{len(steps)} steps for {len(rels)} sigma_rels")
    if len(set(zip(steps, rels))) != len(steps):
        raise ValueError("duplicate (step, sigma_rel) pair among the snapshots")
    take = [i for i, t in enumerate(steps) if t <= t_out]
    if not take:
        raise ValueError(f"no snapshot at or before out_step {t_out}")
    gam = {s: sigma_rel_to_gamma(s) for s in set(rels)}
    g_out = sigma_rel_to_gamma(s_out)
    A = np.array([[profile_dot(steps[i], gam[rels[i]], steps[j], gam[rels[j]]) for j in take] for i in take], dtype=np.float64)
    b = np.array([profile_dot(steps[i], gam[rels[i]], t_out, g_out) for i in take], dtype=np.float64)
    x = np.linalg.solve(A, b)
    out = np.zeros(len(steps), dtype=np.float64)
    out[take] = x / x.sum()
    return out


# ---- tracking ---------------------------------------------------------------------------------------------------------------------
def _check_sigma_rels(sigma_rels):
    rels = [_check_sigma_rel(s) for s in sigma_rels]
    if not 1 <= len(rels) <= L.EMA_MAX_PROFILES:
        raise ValueError(f"{len(rels)} profiles: one launch tracks 1 to {L.EMA_MAX_PROFILES}")
    if len(set(rels)) != len(rels):
        raise ValueError(f"sigma_rels {rels} are not distinct")
    return rels


def _flat_module(model, what):
    inner = getattr(model, "module", model)
    if not isinstance(inner, FlatModule):
        raise NotFlatModuleError(f"{what} needs a vaw_amd FlatModule (e.g. vaw_amd.DiT), got {type(inner).__name__}")
    return inner


def _layout(m):
    return {n: (int(o), int(k), bool(m._flat_cl[n])) for n, (o, k) in m._flat_offsets.items()}


def _same_layout(a, b):
    norm = lambda d: {n: (int(v[0]), int(v[1]), bool(v[2])) for n, v in d.items()}
    return norm(a) == norm(b)


class PowerEMA:
    """K = len(sigma_rels) power-function averages of `model`'s flat parameter buffer (frozen entries included: they are constant,
    so every profile equals them after the first update).  `update()` is two launches on the current stream with no host value in
    them, so it can be captured with the step; everything else reads back on demand."""

    def __init__(self, model, sigma_rels=(0.05, 0.10)):
        inner = _flat_module(model, "PowerEMA")
        self.sigma_rels = _check_sigma_rels(sigma_rels)
        if any(b.is_floating_point() for b in inner.buffers()):
            raise ValueError("PowerEMA averages parameters only: the module has floating-point buffers (as the flat path of trainer.ema)")
        inner.ensure_flat()
        self.model = inner                                   # (a CPU module can be held and serialised; update() needs the GPU)
        self._flat_ptr = inner._flat.data_ptr()
        dev = inner._flat.device
        self.gammas = [sigma_rel_to_gamma(s) for s in self.sigma_rels]
        self.flat = [torch.zeros_like(inner._flat) for _ in self.sigma_rels]
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._gamma = torch.tensor(self.gammas, dtype=torch.float64, device=dev)
        self._coef = torch.zeros(len(self.gammas), dtype=torch.float64, device=dev)

    def update(self):
        m = self.model
        m.ensure_flat()
        if m._flat.data_ptr() != self._flat_ptr:
            raise RuntimeError("the model's flat buffer was rebuilt (moved device / deep-copied) after the PowerEMA was created")
        ops.ema_profiles_coef(self._step, self._gamma, self._coef)
        ops.ema_profiles_update(m._flat, self.flat, self._coef)

    @property
    def step(self):
        """updates so far (reads the device counter back)"""
        return int(self._step.item())

    def coefficients(self):
        """float64 [K]: the c_t of the last update, as the device computed them (reads back)"""
        return self._coef.cpu().numpy().copy()

    def _index(self, sigma_rel):
        s = _check_sigma_rel(sigma_rel)
        if s not in self.sigma_rels:
            raise ValueError(f"sigma_rel {s} is not tracked (tracked: {self.sigma_rels}); posthoc_ema synthesises other widths")
        return self.sigma_rels.index(s)

    def copy_to(self, ema_model, sigma_rel):
        """Write a tracked profile into `ema_model`'s flat buffer: every sampler and evaluator then works on it unchanged."""
        k = self._index(sigma_rel)
        e = _flat_module(ema_model, "copy_to")
        e.ensure_flat()
        if not _same_layout(_layout(e), _layout(self.model)) or e._flat.numel() != self.flat[k].numel():
            raise ValueError("copy_to: the target's flat layout differs from the tracked model's")
        with torch.no_grad():
            e._flat.copy_(self.flat[k])
        e.mark_weights_changed()

    def snapshot(self):
        """A CPU dict of tensors and primitives only (torch.load(weights_only=True) reads it back).  Synchronises."""
        return {"format": SNAPSHOT_FORMAT, "step": self.step, "sigma_rels": list(self.sigma_rels), "layout": _layout(self.model),
                "flat": [f.detach().cpu().clone() for f in self.flat]}

    def save_snapshot(self, path):
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        torch.save(self.snapshot(), path)
        return path

    def state_dict(self):
        return self.snapshot()

    def load_state_dict(self, sd):
        _check_snapshot(sd, "load_state_dict")
        if [float(s) for s in sd["sigma_rels"]] != self.sigma_rels:
            raise ValueError(f"load_state_dict: the state tracks {list(sd['sigma_rels'])}, this PowerEMA {self.sigma_rels}")
        if not _same_layout(sd["layout"], _layout(self.model)) or any(tuple(f.shape) != tuple(self.flat[0].shape) for f in sd["flat"]):
            raise ValueError("load_state_dict: the state's flat layout differs from the tracked model's")
        for mine, theirs in zip(self.flat, sd["flat"]):          # in place: a captured step keeps the addresses
            mine.copy_(theirs.to(torch.float32))
        self._step.fill_(int(sd["step"]))


# ---- reconstruction ---------------------------------------------------------------------------------------------------------------
def _check_snapshot(s, what):
    if not isinstance(s, dict) or s.get("format") != SNAPSHOT_FORMAT:
        raise ValueError(f"{what}: not a PowerEMA snapshot ({SNAPSHOT_FORMAT})")
    if len(s["flat"]) != len(s["sigma_rels"]) or int(s["step"]) < 0:
        raise ValueError(f"{what}: malformed PowerEMA snapshot")
    return s


def _open_snapshot(s, mmap=False):
    if isinstance(s, dict):
        return _check_snapshot(s, "posthoc_ema")
    return _check_snapshot(torch.load(os.fspath(s), map_location="cpu", weights_only=True, mmap=mmap), "posthoc_ema")


def lincomb_fold(tensors, coefficients, device=None, chunk=None, out=None):
    """float32(sum_i coefficients[i] * float64(tensors[i])), accumulated in float64 on the device in the given order: bitwise numpy's
    `acc += c * s.astype(np.float64)` followed by astype(np.float32), whatever `chunk` (elements uploaded at a time; None: a whole
    tensor) is.  `tensors` may be a generator, so they can stream from disk: 8 B per element stay resident, plus the staged chunk."""
    acc = None
    for src, c in zip(tensors, coefficients):
        src = src.detach().reshape(-1)
        if src.dtype != torch.float32:
            raise ValueError(f"lincomb_fold: snapshots are float32, got {src.dtype}")
        if acc is None:
            dev = torch.device(device if device is not None else (out.device if out is not None else "cuda"))
            if dev.type != "cuda":
                raise L.VawError(f"lincomb_fold runs on the GPU only: got device '{dev}' (no CPU fallback exists by design)")
            acc = torch.zeros(src.numel(), dtype=torch.float64, device=dev)
        if src.numel() != acc.numel():
            raise ValueError(f"lincomb_fold: {src.numel()} elements after {acc.numel()}")
        n, step = acc.numel(), int(chunk) if chunk else acc.numel()
        for o in range(0, n, step):
            ops.lincomb_accum_f64(acc[o:o + step], src[o:o + step].to(dev).contiguous(), float(c))
    if acc is None:
        raise ValueError("lincomb_fold: nothing to fold")
    if out is None:
        out = torch.empty(acc.numel(), dtype=torch.float32, device=acc.device)
    ops.f64_to_f32(acc, out)
    return out


def posthoc_ema(snapshots, sigma_rel, step=None, into=None, device=None, return_coefficients=False, chunk=None):
    """The average of relative width `sigma_rel` ending at `step` (default: the last snapshot's), synthesised from PowerEMA snapshots
    (dicts or paths; each holds K profiles, and all n K stored averages at or before `step` take part).  Returns the flat f32 tensor
    on the device; with into=model it is that model's flat buffer, rewritten and marked changed.  The coefficients, in (step,
    sigma_rel) order -- the order of the fold -- are kept on posthoc_ema.last_coefficients, and returned too on request."""
    snapshots = list(snapshots)
    if not snapshots:
        raise ValueError("posthoc_ema: no snapshots")
    entries, layout, numel = [], None, None
    for i, s in enumerate(snapshots):
        snap = _open_snapshot(s, mmap=True)
        if layout is None:
            layout, numel = snap["layout"], snap["flat"][0].numel()
        elif not _same_layout(layout, snap["layout"]) or any(f.numel() != numel for f in snap["flat"]):
            raise ValueError(f"posthoc_ema: snapshot {i} has another flat layout than snapshot 0 (mixed models)")
        entries += [(_check_step(snap["step"], "snapshot step"), _check_sigma_rel(r), i, k) for k, r in enumerate(snap["sigma_rels"])]
        del snap
    entries.sort()
    out_step = max(e[0] for e in entries) if step is None else step
    coefs = posthoc_coefficients([e[0] for e in entries], [e[1] for e in entries], out_step, sigma_rel)
    target = None
    if into is not None:
        target = _flat_module(into, "posthoc_ema(into=...)")
        target.ensure_flat()
        if not _same_layout(_layout(target), layout) or target._flat.numel() != numel:
            raise ValueError("posthoc_ema: `into` has another flat layout than the snapshots")
        L.need_cuda(target._flat)

    def stream():
        opened = (None, None)
        for (t, _, i, k) in (e for e in entries if e[0] <= out_step):
            if opened[0] != i:
                opened = (i, _open_snapshot(snapshots[i]))          # one snapshot in host memory at a time
            yield opened[1]["flat"][k]

    used = [c for e, c in zip(entries, coefs) if e[0] <= out_step]
    with torch.no_grad():
        flat = lincomb_fold(stream(), used, device=device if target is None else target._flat.device, chunk=chunk,
                            out=None if target is None else target._flat)
    if target is not None:
        target.mark_weights_changed()
    posthoc_ema.last_coefficients = coefs
    return (flat, coefs) if return_coefficients else flat


posthoc_ema.last_coefficients = None

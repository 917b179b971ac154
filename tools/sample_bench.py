#!/usr/bin/env python3
"""Sampler timings on one GPU (fixed work, warm-up first, device events or a host clock around a device synchronise).
    python tools/sample_bench.py [--model UNet_32] [--batch 256] [--steps 50] [--iters 200] [--fp32]

For a learn_sigma model under IntervalCFG (scale 2.5, active on part of the chain) over a respaced LEARNED_RANGE chain:
 (a) one guided DDIM step, fused: the stacked model call + vaw_guided_sample_step, the interval decided on the host;
 (b) the same step through the composition of existing pieces (what the step was before the fused kernel): the model call,
     the mean timestep read back from the device, three torch ops, the split halves made contiguous, ops.sample_step.
     Both are also timed WITHOUT the model call (the step's tail alone over rotating buffers larger than the 256 MiB
     Infinity Cache), which is where the byte arithmetic of DESIGN applies;
 (c) vaw_finish_images against the torch expression, f32 and f64, rotating buffers;
 (d) a full Sampler.sample of one batch (DDIM, `--steps` steps), fused and through the composition of (b).
(a) / (b) and the two forms of (c) / (d) alternate inside one timed run.  One JSON line at the end.

With `--solver heun|euler` (EDM sampler), `--solver dpmpp2m|dpmpp2m_sde|expab` (multistep samplers, one evaluation per step) or `--mode flow` (flow SDE sampler, Heun unless `--solver euler`) the run is instead
 (e) one Sampler.sample of `--batches` batches of `--batch` images, `--steps` solver steps, guidance `--guidance`: the time of
     each batch on a host clock (every batch ends in the device-to-host copy of its images), the first `--skip` batches left
     out (tables, workspaces and, with `--graph`, the capture), median / min / max of the rest in ms.  `--fused 0` runs the
     tensor composition (`fused=False`), `--fused 1` the fused solver steps, `--graph` adds args.hip_graph=True.
     `--tree DIR` imports the package from another checkout (built in place), e.g. the parent commit's, which knows
     neither `fused` nor `hip_graph`: pass neither there.

With `--seeded` beside them the run is
 (i) the same Sampler.sample four times over, twice (the second round is reported): noise from the torch generator and from
     SeededNoise (args.sample_seed), each eager and as a captured graph (args.hip_graph): median / min ms per batch of each;
     then the draw alone on `--batch` x C x S x S, float32 and float64: `normal_()` of the torch generator against
     ops.randn_seeded in us, device events over `--iters` calls on rotating destinations.

With `--solver rk45` the run is
 (f) flow_ode_sample(solver="rk45") over a stand-in network (0.6 tanh(2x) + 0.5 sin(12 t) + 0.02 y: three tensor operations, so
     the time is the solver's own) on `--batch` x 4 x S x S noise (S = `--image-size` or 32), linear path, VELOCITY,
     `--rtol` / `--atol`: attempts, network evaluations and read-backs of a call, and the median ms per attempt of `--repeats`
     calls, fused (vaw_rk_stage) and as the tensor composition (`fused=False`) alternating, each after a warm-up call.

With `--dpm-kernel` the run is
 (h) vaw_dpm_step alone on `--batch` x 4 x S x S (S = `--image-size` or 64) float64 states over rotating sets larger than the
     256 MiB Infinity Cache, device events over `--iters` calls: unguided with two nodes (dpmpp2m: 8 + 4 + 4 read, 8 + 4 + 4
     written = 32 B/element) and guided with three nodes and noise (52 B/element), in us and algorithmic TB/s, checked once
     against the tensor composition.

With `--logp` the run is
 (g) one flow_log_likelihood sweep (`--steps` grid points, `--solver euler|heun`, cosine path, VELOCITY) of `--batch` samples
     through `--model`: the median ms of `--repeats` sweeps with the full backward per evaluation (the model wrapped so that it
     shows no input_grad_only) and with input_grad_only(), alternating after a warm-up sweep of each, and whether both give the
     same logp bit for bit; then the pass after a network call alone (Heun's second stage on max(`--batch`, 1024) rows):
     vaw_flow_logp_stage against the tensor composition in us, device events over `--iters` calls on rotating buffers."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

_tree = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--tree" or a.startswith("--tree=")]
sys.path.insert(0, os.path.abspath(_tree[0]) if _tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaw_amd  # noqa: E402
from vaw_amd import ops  # noqa: E402

SCALE = 2.5


class CompositionCFG(torch.nn.Module):
    """IntervalCFG without guided_halves: the predicate read back from the device and three tensor operations."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg

    def forward(self, x, t, **kw):
        if not self.cfg.guidance_active(float(t.float().mean())):
            return self.cfg.model(x, t, **kw)
        n, y = x.shape[0], kw["y"]
        out = self.cfg.model(x.repeat(2, 1, 1, 1), t.repeat(2), **{**kw, "y": torch.cat((y, y.new_full(y.shape, self.cfg.null_label)))})
        out = out[0] if isinstance(out, tuple) else out
        return out[n:] + self.cfg.guidance_scale * (out[:n] - out[n:])


class CompositionSampler(vaw_amd.Sampler):
    def _build_cfg_model(self, num_classes):
        return CompositionCFG(super()._build_cfg_model(num_classes)).eval()

    def _inverse_normalize(self, samples):
        return ((samples + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def events_us(fns, iters):
    """Mean time per call in us: the callables alternate, warm-up of each first."""
    for f in fns:
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def wall_pair(fa, fb, repeats):
    """Medians in seconds of two callables that end in a device synchronise, alternating."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(repeats):
        for f, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]


def build_model(a, learn_sigma=True):
    dt = "fp32" if a.fp32 else "bf16"
    if a.model.startswith("DiT"):
        model = vaw_amd.DiT_models[a.model.replace("_", "-")](image_size=a.image_size or 32, patch_size=a.patch, in_channels=4, class_dropout_prob=0.1,
                                                              num_classes=a.num_classes, learn_sigma=learn_sigma, compute_dtype=dt)
        C, H = 4, a.image_size or 32
    else:
        model = getattr(vaw_amd, a.model)(num_classes=a.num_classes, class_cond=True, learn_sigma=learn_sigma, drop_label_prob=0.1, compute_dtype=dt)
        C, H = model.in_channels, model.image_size
    model = model.to("cuda").eval()
    with torch.no_grad():
        for p in model.parameters():          # zero-initialised output layers would make every step trivial
            if p.requires_grad:
                p.add_(torch.randn_like(p) * 0.02)
    if hasattr(model, "mark_weights_changed"):
        model.mark_weights_changed()
    return model, C, H


def solver_run(a, model, C, H, graph, seeded):
    """Sorted per-batch times in ms of one Sampler.sample of `--batches` batches, the first `--skip` left out."""
    flow = a.mode == "flow"
    args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=not flow, p2_gamma=1, p2_k=1, time_dist=["uniform"], cpu_rng=False,
                           in_chans=3 if C == 3 else 4, class_cond=True, parallel=False, class_labels=None, amp=False, latent_scale=0.18215,
                           guidance_scale=a.guidance, interval=(-1.0, -1.0), model_mode="flow" if flow else "diffusion", solver=a.solver or "heun",
                           sample_steps=a.steps, discretization="edm", schedule="linear", scaling="none", path_type="linear" if flow else "cosine",
                           mean_type="VELOCITY" if flow else "EPSILON", sampler_type="sde")
    if graph:
        args.hip_graph = True
    if seeded:
        args.sample_seed = 1234
    diff = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY) if flow else None
    s = vaw_amd.Sampler(args, torch.device("cuda"), model, diff, **(dict(decode_fn=(lambda z: z[:, :3])) if C == 4 else {}))
    stamps, gather = [], s._gather_samples

    def timed_gather(*g):
        gather(*g)                          # ends in the images' copy to the host: the batch is done
        stamps.append(time.perf_counter())
    s._gather_samples = timed_gather
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    s.sample(a.batch * a.batches, a.batch, H, a.num_classes)
    return sorted(1e3 * (t1 - t0) for t0, t1 in zip(stamps[a.skip:-1], stamps[a.skip + 1:]))


def solver_bench(a):
    """(e): per-batch time of Sampler.sample through the EDM / flow solvers; (i) with --seeded."""
    import functools
    flow = a.mode == "flow"
    solver = a.solver or "heun"
    torch.manual_seed(0)
    model, C, H = build_model(a, learn_sigma=not flow)
    if a.fused is not None:
        import vaw_amd.sampler as sm
        for name in ("edm_sample", "dpm_sample", "flow_sde_sample", "flow_ode_sample"):
            if not hasattr(sm, name):          # an older --tree
                continue
            setattr(sm, name, functools.partial(getattr(sm, name), fused=bool(a.fused)))
    evals = (2 * a.steps - 1 if solver == "heun" else a.steps)          # euler and the multistep solvers: one per step
    res = {"part": "i" if a.seeded else "e", "model": a.model, "dtype": "fp32" if a.fp32 else "bf16", "mode": a.mode, "solver": solver,
           "steps": a.steps, "batch": a.batch, "guidance": a.guidance, "fused": a.fused, "tree": a.tree or ".", "evaluations_per_batch": evals}
    if not a.seeded:
        ms = solver_run(a, model, C, H, a.graph, False)
        res.update({"graph": bool(a.graph), "batches_timed": len(ms), "ms_per_batch_median": ms[len(ms) // 2], "ms_per_batch_min": ms[0],
                    "ms_per_batch_max": ms[-1]})
        return print(json.dumps(res))
    # (i): the four runs one after the other, twice, the second round reported (the first warms the allocator and the tables)
    for _ in range(2):
        for graph in (False, True):
            for seeded in (False, True):
                ms = solver_run(a, model, C, H, graph, seeded)
                name = f"{'seeded' if seeded else 'torch'}_{'graph' if graph else 'eager'}"
                res.update({f"{name}_ms_per_batch_median": ms[len(ms) // 2], f"{name}_ms_per_batch_min": ms[0], "batches_timed": len(ms)})
    # the draw alone, over rotating destinations larger than the 256 MiB Infinity Cache: 4 (8) bytes written per element
    shape = (a.batch, 3 if C == 3 else 4, H, H)
    seeds = torch.arange(a.batch, device="cuda")
    res["draw_elements"] = elems = a.batch * shape[1] * H * H
    with torch.no_grad():
        for dt, nm in ((torch.float32, "f32"), (torch.float64, "f64")):
            outs = [torch.empty(shape, device="cuda", dtype=dt) for _ in range(max(2, int(600e6 // (elems * dt.itemsize)) + 1))]
            us_t = events_us([(lambda o=o: o.normal_()) for o in outs], a.iters)
            us_s = events_us([(lambda o=o, i=i: ops.randn_seeded(seeds, shape, i, dtype=dt, out=o)) for i, o in enumerate(outs)], a.iters)
            res.update({f"draw_{nm}_torch_us": us_t, f"draw_{nm}_seeded_us": us_s, f"draw_{nm}_seeded_Gelements_per_s": elems / us_s / 1e3})
            del outs
    print(json.dumps(res))


def dpm_kernel_bench(a):
    """(h): vaw_dpm_step against its bytes."""
    from vaw_amd import samplers
    S, N = a.image_size or 64, a.batch
    shape = (N, 4, S, S)
    net = vaw_amd.EDMDenoiser(torch.nn.Identity(), S, 4).to("cuda")
    lo, hi = samplers._edm_sigma_range(net, "edm", None, None, 1e-3)
    coef = samplers._dpm_tables(net, torch.device("cuda"), N, 18, lo, hi, 7, "dpmpp2m_sde", None, "edm", 1e-3, 1.0, 1.0).coef.clone()
    coef[:, 3] = 0.125
    elems = N * 4 * S * S
    sets = []
    for _ in range(max(2, int(600e6 // (elems * 52)) + 1)):
        sets.append(dict(x=torch.randn(shape, device="cuda", dtype=torch.float64), nz=torch.randn(shape, device="cuda", dtype=torch.float64),
                         out=torch.randn((2 * N, *shape[1:]), device="cuda"), d=[torch.randn(shape, device="cuda") for _ in range(3)],
                         buf=torch.empty((2 * N, *shape[1:]), device="cuda")))
    row = 9

    def plain(s):
        return lambda: ops.dpm_step("EPSILON", False, s["out"][:N], None, 1.0, s["x"], s["d"][1], None, None, coef, row, x_out=s["x"],
                                    d0_out=s["d"][0], model_in=s["buf"][:N])

    def full(s):
        return lambda: ops.dpm_step("EPSILON", False, s["out"][:N], s["out"][N:], SCALE, s["x"], s["d"][1], s["d"][2], s["nz"], coef, row,
                                    x_out=s["x"], d0_out=s["d"][0], model_in=s["buf"][:N], model_in_dup=s["buf"][N:])

    s0 = sets[0]
    o = s0["out"][N:] + SCALE * (s0["out"][:N] - s0["out"][N:])
    sigma = coef[row, 5].float()
    den = s0["x"].float() - sigma * o
    ref = coef[row, 0] * s0["x"] + coef[row, 1] * den.double()
    ref = ref + coef[row, 2] * s0["d"][1].double()
    ref = ref + coef[row, 3] * s0["d"][2].double()
    ref = ref + coef[row, 4] * s0["nz"]
    full(s0)()
    assert torch.equal(s0["x"], ref) and torch.equal(s0["d"][0], den), "vaw_dpm_step differs from the composition"
    del o, den, ref
    res = {"part": "h", "batch": N, "elements": elems, "rotating_sets": len(sets)}
    for name, mk, nbytes in (("two_nodes_unguided", plain, 32), ("three_nodes_guided_noise", full, 52)):
        fns = [mk(s) for s in sets]
        events_us(fns, 2 * len(fns))
        us = events_us(fns, a.iters)
        res[f"{name}_us"], res[f"{name}_bytes_per_element"], res[f"{name}_algorithmic_TBps"] = us, nbytes, nbytes * elems / us / 1e6
    print(json.dumps(res))


def rk45_bench(a):
    """(f): the adaptive flow-ODE solver around a stand-in network, fused against the tensor composition."""
    S = a.image_size or 32
    args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=False, p2_gamma=1, p2_k=1, path_type="linear")
    fm = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY)
    col = lambda v, x: v.reshape(-1, 1, 1, 1).to(x.dtype)
    standin = lambda x, t, y=None, **kw: 0.6 * torch.tanh(2 * x) + 0.5 * torch.sin(12 * col(t, x)) + 0.02 * col(y, x)
    torch.manual_seed(1)
    x0 = torch.randn(a.batch, 4, S, S, device="cuda")
    y = torch.arange(a.batch, device="cuda") % a.num_classes
    res = {"part": "f", "solver": "rk45", "batch": a.batch, "elements_per_sample": 4 * S * S, "rtol": a.rtol, "atol": a.atol}
    outs = {}

    def run(fused):
        outs[fused] = vaw_amd.flow_ode_sample(fm, standin, x0, solver="rk45", rtol=a.rtol, atol=a.atol, fused=fused, y=y)
        return dict(fm.last_ode_stats)

    stats = {fused: run(fused) for fused in (True, False)}          # warm-up
    t_f, t_c = wall_pair(lambda: run(True), lambda: run(False), max(a.repeats, 5))
    for name, fused, t in (("fused", True, t_f), ("composition", False, t_c)):
        st = stats[fused]
        attempts = st["accepted"] + st["rejected"]
        res.update({f"{name}_attempts": attempts, f"{name}_accepted": st["accepted"], f"{name}_nfev": st["nfev"], f"{name}_readbacks": st["readbacks"],
                    f"{name}_ms_per_call": 1e3 * t, f"{name}_ms_per_attempt": 1e3 * t / attempts})
    res["bitwise_equal"] = bool(torch.equal(outs[True], outs[False]))
    res["max_abs_diff"] = float((outs[True].double() - outs[False].double()).abs().max())
    print(json.dumps(res))


class FullBackward(torch.nn.Module):
    """The model without its input_grad_only(): flow_log_likelihood then runs the full backward per evaluation."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x, t, **kw):
        return self.model(x, t, **kw)


def logp_bench(a):
    """(g): one flow_log_likelihood sweep, with the full backward per evaluation and with input_grad_only()."""
    torch.manual_seed(0)
    model, C, H = build_model(a, learn_sigma=False)
    args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=False, p2_gamma=1, p2_k=1, path_type="cosine")
    fm = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY)
    x = torch.randn(a.batch, C, H, H, device="cuda")
    y = torch.arange(a.batch, device="cuda") % a.num_classes
    solver = a.solver or "heun"
    full = FullBackward(model).eval()
    outs = {}

    def run(m, name):
        outs[name] = fm.calc_bpd(m, x, num_steps=a.steps, solver=solver, generator=torch.Generator(device="cuda").manual_seed(1), y=y)

    t_full, t_only = wall_pair(lambda: run(full, "full"), lambda: run(model, "only_dx"), max(a.repeats, 3))
    nfev = outs["only_dx"]["nfev"]
    # the pass after a network call alone: Heun's second stage (reads out, x_1, g, eps, x, k_0; writes k_1, x_new: 32 B/element),
    # the kernel against the tensor composition, over rotating sets larger than the 256 MiB Infinity Cache
    R, n = max(a.batch, 1024), C * H * H
    A, B, h, b = 0.25, -1.5, 0.125, (0.5, 0.5)
    coef = torch.tensor([[A, B, 0.0, 0.0]], device="cuda")
    sets = []
    with torch.no_grad():
        for _ in range(max(2, int(400e6 // (R * n * 4 * 8)) + 1)):
            t = lambda: torch.randn(R, C, H, H, device="cuda")
            k = torch.randn(ops.RK_STAGES, R, C, H, H, device="cuda")          # (only slots 0 and 1 are touched)
            sets.append(dict(out=t(), g=t(), eps=torch.randint(0, 2, (R, C, H, H), device="cuda").float() * 2 - 1, x=t(), xs=t(), k=k,
                             d=torch.randn(ops.RK_STAGES, R, device="cuda", dtype=torch.float64), xn=t(),
                             delta=torch.zeros(R, device="cuda", dtype=torch.float64)))
        partials = torch.empty(ops.rk_partial_count(R, n), device="cuda", dtype=torch.float64)

        def fused(s):
            return lambda: ops.flow_logp_stage(1, s["out"], s["g"], s["eps"], s["x"], s["xs"], coef, 0, s["k"], s["d"], b, h, x_out=s["xn"],
                                               delta=s["delta"], partials=partials)

        def comp(s):
            def run_comp():
                kv = A * s["xs"] + B * s["out"]
                dv = A * n + B * (s["eps"].to(torch.float64) * s["g"].to(torch.float64)).flatten(1).sum(1)
                xn = s["x"] + h * (b[0] * s["k"][0] + b[1] * kv)
                return kv, xn, s["delta"] + h * (b[0] * s["d"][0] + b[1] * dv)
            return run_comp

        fused(sets[0])()
        kv, xn, _ = comp(sets[0])()
        assert torch.equal(sets[0]["k"][1], kv) and torch.equal(sets[0]["xn"], xn), "the stage kernel differs from the composition"
        stage_us = events_us([fused(s) for s in sets], a.iters)
        comp_us = events_us([comp(s) for s in sets], a.iters)
    print(json.dumps({"part": "g", "model": a.model, "stage_rows": R, "stage_elements_per_row": n, "stage_kernel_us": stage_us,
                      "stage_composition_us": comp_us, "stage_kernel_algorithmic_TBps": 32.0 * R * n / stage_us / 1e6, "dtype": "fp32" if a.fp32 else "bf16", "batch": a.batch, "grid_points": a.steps, "solver": solver,
                      "evaluations": nfev, "full_backward_ms_per_sweep": 1e3 * t_full, "input_grad_only_ms_per_sweep": 1e3 * t_only,
                      "full_backward_ms_per_evaluation": 1e3 * t_full / nfev, "input_grad_only_ms_per_evaluation": 1e3 * t_only / nfev,
                      "logp_bitwise_equal": bool(torch.equal(outs["full"]["logp"], outs["only_dx"]["logp"])),
                      "bpd_mean": float(outs["only_dx"]["bpd"].mean())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logp", action="store_true",
                    help="(g): time one flow_log_likelihood sweep of --steps grid points (--solver euler|heun, default heun) with the full "
                         "backward per evaluation and with input_grad_only()")
    ap.add_argument("--solver", choices=["heun", "euler", "dpmpp2m", "dpmpp2m_sde", "expab", "rk45"], default=None,
                    help="(e): time Sampler.sample through this EDM / multistep / flow solver; rk45: (f), the adaptive flow-ODE solver")
    ap.add_argument("--dpm-kernel", action="store_true", help="(h): vaw_dpm_step alone against its bytes")
    ap.add_argument("--rtol", type=float, default=1e-3, help="(f)")
    ap.add_argument("--atol", type=float, default=1e-6, help="(f)")
    ap.add_argument("--mode", choices=["diffusion", "flow"], default="diffusion")
    ap.add_argument("--fused", type=int, choices=[0, 1], default=None, help="(e): 0 = the tensor composition, 1 = the fused solver steps")
    ap.add_argument("--graph", action="store_true", help="(e): args.hip_graph=True")
    ap.add_argument("--seeded", action="store_true",
                    help="(i): torch generator against SeededNoise (args.sample_seed), eager and captured, for --solver (default heun) / --mode flow")
    ap.add_argument("--guidance", type=float, default=1.0, help="(e): guidance scale (1.0, the reference's default: unguided)")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--tree", default=None, help="import vaw_amd from this checkout instead of the one the script lives in")
    ap.add_argument("--model", default="UNet_32")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=0)
    ap.add_argument("--patch", type=int, default=2)
    ap.add_argument("--num-classes", type=int, default=10)
    ap.add_argument("--fp32", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py measures on the GPU only")
    if a.logp:
        return logp_bench(a)
    if a.dpm_kernel:
        with torch.no_grad():
            return dpm_kernel_bench(a)
    if a.solver == "rk45":
        with torch.no_grad():
            return rk45_bench(a)
    if a.solver or a.mode == "flow" or a.seeded:
        return solver_bench(a)
    torch.manual_seed(0)
    model, C, H = build_model(a)
    N, n = a.batch, C * H * H
    args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=True, p2_gamma=1, p2_k=1, time_dist=["uniform"], cpu_rng=False,
                           in_chans=3 if C == 3 else 4, class_cond=True, parallel=False, class_labels=None, amp=False, latent_scale=0.18215,
                           guidance_scale=SCALE, interval=(100.0, 900.0), model_mode="diffusion", solver="ddim")
    d = vaw_amd.SpacedDiffusion(use_timesteps=vaw_amd.space_timesteps(1000, str(a.steps)), args=args, betas=vaw_amd.get_named_beta_schedule("linear", 1000),
                                model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.LEARNED_RANGE,
                                loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    res = {"model": a.model, "dtype": "fp32" if a.fp32 else "bf16", "batch": N, "elements_per_sample": n, "chain_steps": a.steps}

    with torch.no_grad():
        # (a) / (b): the step's tail alone, rotating sets
        i_mid = a.steps // 2
        t = torch.full((N,), i_mid, device="cuda", dtype=torch.long)
        coef = d._sample_rows(t)
        nset = max(2, int(400e6 // (N * n * 4 * 8)) + 1)
        sets = []
        for _ in range(nset):
            out = torch.randn(2 * N, 2 * C, H, H, device="cuda")
            out[:, C:].clamp_(-1, 1)
            sets.append((out, torch.randn(N, C, H, H, device="cuda"), torch.randn(N, C, H, H, device="cuda")))

        def fused_tail(s):
            out, x, nz = s
            return lambda: ops.guided_sample_step(2, out[:N, :C], out[N:, :C], out[:N, C:], out[N:, C:], SCALE, x, nz, coef, 0, 2, True, 0.0)

        def comp_tail(s):
            out, x, nz = s

            def run():
                float(t.float().mean())                                    # the per-step read-back of the interval predicate
                comb = out[N:] + SCALE * (out[:N] - out[N:])
                m, v = torch.split(comb, C, dim=1)
                return ops.sample_step(2, m.contiguous(), v.contiguous(), x, nz, coef, 0, 2, True, 0.0)
            return run

        got, ref = fused_tail(sets[0])(), comp_tail(sets[0])()
        assert all(torch.equal(got[k], ref[k]) for k in ref), "fused step differs from the composition"
        fs, cs = [fused_tail(s) for s in sets], [comp_tail(s) for s in sets]
        both = [f for pair in zip(fs, cs) for f in pair]
        events_us(both, 2 * len(both))                                       # warm-up of every set
        res["a_tail_fused_us"] = events_us(fs, a.iters)
        res["b_tail_composition_us"] = events_us(cs, a.iters)
        res["tail_elements"] = N * n
        res["a_tail_fused_algorithmic_TBps"] = 32.0 * N * n / res["a_tail_fused_us"] / 1e6

        # (a) / (b): the whole guided step, model call included
        y = torch.randint(0, a.num_classes, (N,), device="cuda")
        cfg = vaw_amd.IntervalCFG(model, a.num_classes, SCALE, args.interval, True).eval()
        comp_cfg = CompositionCFG(cfg).eval()
        x = torch.randn(N, C, H, H, device="cuda")
        assert cfg.guidance_active(d._host_model_time(i_mid))
        step_f = lambda: d._reverse_step(2, cfg, x, t, True, None, None, {"y": y}, t_host=i_mid)
        step_c = lambda: d._reverse_step(2, comp_cfg, x, t, True, None, None, {"y": y})
        for _ in range(3):
            step_f(), step_c()
        it = max(10, a.iters // 10)
        res["a_step_fused_us"] = events_us([step_f], it)
        res["b_step_composition_us"] = events_us([step_c], it)
        res["a_step_fused_us_again"] = events_us([step_f], it)

        # (c) finish_images against the torch expression
        torch_finish = lambda v: ((v + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        for dt, nm in ((torch.float32, "f32"), (torch.float64, "f64")):
            imgs = [torch.rand(N, 3, H, H, device="cuda", dtype=dt) * 3 - 1.5 for _ in range(max(2, int(400e6 // (N * 3 * H * H * dt.itemsize)) + 1))]
            assert torch.equal(ops.finish_images(imgs[0]), torch_finish(imgs[0]))
            res[f"c_finish_{nm}_us"] = events_us([(lambda v=v: ops.finish_images(v)) for v in imgs], a.iters)
            res[f"c_torch_{nm}_us"] = events_us([(lambda v=v: torch_finish(v)) for v in imgs], a.iters)
            del imgs

    # (d) a full Sampler.sample of one batch
    kw = dict(decode_fn=(lambda z: z[:, :3])) if C == 4 else {}
    fused = vaw_amd.Sampler(args, torch.device("cuda"), model, d, **kw)
    comp = CompositionSampler(args, torch.device("cuda"), model, d, **kw)
    run = lambda s: (lambda: (torch.manual_seed(1), s.sample(N, N, H, a.num_classes)))
    res["d_sample_fused_s"], res["d_sample_composition_s"] = wall_pair(run(fused), run(comp), a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""flow_ode_sample(solver="rk45") on the GPU: vaw_rk_stage bitwise the tensor composition of every stage, the scaled sums of
squares against float64 torch and bitwise from run to run, the fused loop against fused=False on the device (stand-in and
tiny DiT under IntervalCFG) and against the scipy fixture, its statistics, and Sampler."""
import itertools
import os

import numpy as np
import pytest
import torch

import rk45_cases as rc
from conftest import GOLDEN
from sampler_cases import Standin, sampler_args
from test_gpu_sampler_solvers import LAYOUTS, SCALE, SHAPE_IDS, SHAPES, differ, flow_fm, model_for, model_output

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops, samplers

DEV = "cuda"
FIX = np.load(os.path.join(GOLDEN, "rk45.npz"))
RTOL, ATOL, H = 1e-4, 1e-5, -0.137
SLOTS = [3, 0, 6, 1, 5, 2, 4]          # stage -> slot of k: not the identity, as after accepted steps


def finished(partials, count):
    return float(ops.rk_sumsq_finish(partials, count, torch.zeros(1, dtype=torch.float64, device=DEV)))


# ---- vaw_rk_stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rk_stage_is_bitwise_the_tensor_composition(shape, layout):
    N = shape[0]
    g = torch.Generator().manual_seed(sum(shape) + 5)
    x, x_stage, x_new = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    k0 = torch.randn((7, *shape), generator=g).to(DEV)
    out = model_output(shape, layout, 31 + len(layout))
    times = [0.83 + c * H for c in samplers._DP_C[:6]] + [0.83 + H]
    count = ops.rk_partial_count(N, x[0].numel())
    assert count == N * (4 if shape == (3, 4, 32, 32) else 1)
    new = lambda rows=N: torch.full((rows, *shape[1:]), 7.0, device=DEV)
    for (mean_type, path_type), guided in itertools.product(zip(ops.FLOW_MEAN, ("cosine", "linear", "cosine", "linear_logsnr")), (True, False)):
        fm = flow_fm(path_type, mean_type)
        be = samplers._RK45Fused(fm, None, x, RTOL, ATOL, {})
        coef, trows, _ = be.tables(times)
        assert coef.shape == (7, ops.FLOW_COLS) and trows.shape == (7, 2 * N)
        cond, uncond = out[:N], (out[N:] if guided else None)
        o = uncond + SCALE * (cond - uncond) if guided else cond
        for i in range(7):
            what = (mean_type, path_type, guided, i)
            xs = x if i == 0 else x_stage
            tb = fm.expand_t_like_x(torch.tensor(times[i], dtype=torch.float64, device=DEV), x)
            assert torch.equal(trows[i], tb.view(N).repeat(2))
            k_ref = samplers._flow_fields(fm, o, xs, tb)[0]
            ks = [k_ref if j == i else k0[SLOTS[j]] for j in range(7)]
            k = k0.clone()
            if i < 6:
                coeffs = samplers._DP_A[i + 1]
                buf = new(2 * N)
                ops.rk_stage(i, mean_type, cond, uncond, SCALE, x, None if i == 0 else x_stage, coef, i, k, SLOTS, coeffs, H, buf[:N], buf[N:])
                ref = x + H * samplers._rk_combine(coeffs, ks)
                assert torch.equal(buf[:N], ref) and torch.equal(buf[N:], ref), (what, "state", differ(buf[:N], ref))
                assert bool(torch.isfinite(ref).all())
            else:
                partials = torch.full((count + 1,), 7.0, dtype=torch.float64, device=DEV)
                ops.rk_stage(i, mean_type, cond, uncond, SCALE, x, x_stage, coef, i, k, SLOTS, samplers._DP_E, H, x_new=x_new, atol=ATOL, rtol=RTOL,
                             partials=partials)
                r = (H * samplers._rk_combine(samplers._DP_E, ks)) / (ATOL + RTOL * torch.maximum(x.abs(), x_new.abs()))
                ref = float((r.double() ** 2).sum())
                got = finished(partials, count)
                assert float(partials[count]) == 7.0 and abs(got - ref) <= 1e-12 * ref, (what, "error", got, ref)
            assert torch.equal(k[SLOTS[i]], k_ref), (what, "k", differ(k[SLOTS[i]], k_ref))
            untouched = [s for s in range(7) if s != SLOTS[i]]
            assert torch.equal(k[untouched], k0[untouched]), (what, "another slot was written")
        # k only (the evaluations of the first-step selection), and in place over the stage state
        k = k0.clone()
        ops.rk_stage(1, mean_type, cond, uncond, SCALE, x, x_stage, coef, 3, k, SLOTS, (), 0.0)
        tb = fm.expand_t_like_x(torch.tensor(times[3], dtype=torch.float64, device=DEV), x)
        assert torch.equal(k[SLOTS[1]], samplers._flow_fields(fm, o, x_stage, tb)[0])
        k, inplace = k0.clone(), x_stage.clone()
        ops.rk_stage(2, mean_type, cond, uncond, SCALE, x, inplace, coef, 2, k, SLOTS, samplers._DP_A[3], H, x_out=inplace)
        tb = fm.expand_t_like_x(torch.tensor(times[2], dtype=torch.float64, device=DEV), x)
        ks = [samplers._flow_fields(fm, o, x_stage, tb)[0] if j == 2 else k0[SLOTS[j]] for j in range(3)]
        assert torch.equal(inplace, x + H * samplers._rk_combine(samplers._DP_A[3], ks)), (mean_type, "in place")
    # without a network output: k as it stands -- the Euler trial's coefficient vector, and a step tried again
    for stage, coeffs in ((0, (1.0,)), (0, samplers._DP_A[1]), (4, samplers._DP_A[5])):
        k, buf = k0.clone(), new(2 * N)
        ops.rk_stage(stage, "VELOCITY", None, None, 1.0, x, None, None, 0, k, SLOTS, coeffs, H, buf[:N], buf[N:])
        ref = x + H * samplers._rk_combine(coeffs, [k0[SLOTS[j]] for j in range(7)])
        assert torch.equal(buf[:N], ref) and torch.equal(buf[N:], ref) and torch.equal(k, k0), (stage, coeffs, differ(buf[:N], ref))
    with pytest.raises(vaw_amd.VawError, match="row 7 outside"):
        ops.rk_stage(0, "VELOCITY", out[:N], None, 1.0, x, None, coef, 7, k, SLOTS, (0.2,), H, new())


# ---- vaw_rk_scaled_sumsq + finish -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_scaled_sumsq_matches_float64_torch_and_is_bitwise_reproducible(shape):
    N = shape[0]
    g = torch.Generator().manual_seed(sum(shape) + 6)
    u, v, a, b = (torch.randn(shape, generator=g).to(DEV) for _ in range(4))
    shifted = torch.empty(u.numel() + 1, device=DEV)[1:].view(shape).copy_(u)          # scalar accesses, the same partial sums
    count = ops.rk_partial_count(N, u[0].numel())
    assert u.numel() <= 12288
    for uu, vv, bb in ((u, None, None), (u, v, None), (u, v, b), (u, None, b), (shifted, v, b)):
        d = uu - vv if vv is not None else uu
        m = torch.maximum(a.abs(), bb.abs()) if bb is not None else a.abs()
        ref = float(((d / (ATOL + RTOL * m)).double() ** 2).sum())
        runs = []
        for _ in range(2):
            partials = torch.full((count + 1,), 7.0, dtype=torch.float64, device=DEV)
            ops.rk_scaled_sumsq(uu, vv, a, bb, ATOL, RTOL, partials)
            runs.append((finished(partials, count), partials.clone()))
        (got, p0), (again, p1) = runs
        assert abs(got - ref) <= 1e-12 * ref, (got, ref)
        assert got == again and torch.equal(p0, p1) and float(p0[count]) == 7.0
    with pytest.raises(vaw_amd.VawError, match="partials"):
        ops.rk_scaled_sumsq(u, None, a, None, ATOL, RTOL, torch.zeros(max(count - 1, 0), dtype=torch.float64, device=DEV))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def both_ways(fm, model, x0, **kw):
    res = []
    for fused in (False, True):
        x = vaw_amd.flow_ode_sample(fm, model, x0, solver="rk45", fused=fused, **kw)
        res.append((x, dict(fm.last_ode_stats)))
    (ref, rs), (got, gs) = res
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape and bool(torch.isfinite(ref).all())
    assert (gs["accepted"], gs["rejected"]) == (rs["accepted"], rs["rejected"]), (gs, rs)
    bound = 4 * 2.0 ** -23 * max(1.0, float(ref.abs().max()))
    diff = float((got.double() - ref.double()).abs().max())
    print(f"fused vs composition: {differ(got, ref)}; bound {bound:.3e}; accepted {gs['accepted']} rejected {gs['rejected']}")
    assert diff <= bound, differ(got, ref)
    attempts = gs["accepted"] + gs["rejected"]
    assert gs["nfev"] == rs["nfev"] == 2 + 6 * attempts + 1 and gs["readbacks"] <= attempts + 2
    return ref, gs


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_fused_loop_reproduces_the_fixture_and_the_composition(case):
    path, mean, shape = case
    cid = rc.case_id(case)
    x0, y = rc.inputs(shape, DEV)
    fm = rc.flow(path, mean)
    both_ways(fm, rc.standin, x0, rtol=rc.RTOL, atol=rc.ATOL, y=y)
    st = fm.last_ode_stats          # of the fused run
    assert (st["accepted"], st["accepted"] + st["rejected"]) == (int(FIX[f"{cid}/accepted"]), int(FIX[f"{cid}/attempts"])), st
    got = vaw_amd.flow_ode_sample(fm, rc.standin, x0, solver="rk45", rtol=rc.RTOL, atol=rc.ATOL, y=y)          # fused=None: the kernels
    diff = float(np.abs(got.double().cpu().numpy() - FIX[f"{cid}/final"]).max())
    print(f"{cid}: fused max |diff| vs scipy {diff:.3e}, the composition's on the CPU {float(FIX[f'{cid}/dist']):.3e}")
    assert diff <= 4 * float(FIX[f"{cid}/dist"])          # (4: the device's tanh / sin against the host's)


def stage_times(stats):
    return [t + c * h for t, h, _ in stats["trace"] for c in samplers._DP_C]


@pytest.mark.parametrize("guidance", ["always", "interval"])
@pytest.mark.parametrize("name", ["standin", "dit"])
def test_fused_loop_under_guidance_is_the_composition(name, guidance):
    scale, interval = {"always": (SCALE, (-1.0, -1.0)), "interval": (1.8, (0.2, 0.7))}[guidance]
    if name == "dit":
        model, size = model_for("dit", False)
        shape, y = (3, 3, size, size), torch.tensor([1, 5, 9], device=DEV)
    else:
        model, shape, y = Standin(rc.standin), (3, 3, 5, 5), torch.tensor([1, 4, 7], device=DEV)
    calls = []
    cfg = vaw_amd.IntervalCFG(model, 10, scale, interval, True)
    hook = model.register_forward_pre_hook(lambda m, a: calls.append(a[0].shape[0]))
    fm = flow_fm("linear", "VELOCITY")
    torch.manual_seed(11)
    x0 = torch.randn(shape, device=DEV)
    try:
        _, st = both_ways(fm, cfg, x0, rtol=1e-3, atol=1e-4, y=y)
    finally:
        hook.remove()
    times = stage_times(st)
    assert guidance == "always" or all(min(abs(t - e) for e in interval) >= 1e-3 for t in times), "a stage time next to an edge of the interval"
    half = len(calls) // 2
    assert calls[:half] == calls[half:] and half == st["nfev"]          # the same calls, guided at the same evaluations
    stacked = sum(b == 2 * shape[0] for b in calls[:half])
    assert stacked == half if guidance == "always" else 0 < stacked < half


def test_fused_loop_without_guidance_and_with_a_scale_of_one():
    x0, y = rc.inputs((2, 4, 8, 8), DEV)
    fm = rc.flow("cosine", "VELOCITY")
    ref, _ = both_ways(fm, rc.standin, x0, rtol=1e-3, atol=1e-5, y=y)
    off = vaw_amd.IntervalCFG(Standin(rc.standin), 10, 1.0, (-1.0, -1.0), True)          # never active: the batch is not stacked
    got = vaw_amd.flow_ode_sample(fm, off, x0, solver="rk45", rtol=1e-3, atol=1e-5, y=y)
    assert torch.equal(got, vaw_amd.flow_ode_sample(fm, rc.standin, x0, solver="rk45", rtol=1e-3, atol=1e-5, y=y))
    with pytest.raises(FloatingPointError, match="t=1.0"):
        vaw_amd.flow_ode_sample(fm, lambda x, t, **kw: x * float("nan"), x0, solver="rk45")


# ---- Sampler ------------------------------------------------------------------------------------------------------------------------
def test_sampler_rk45_returns_the_bytes_of_the_composition_and_refuses_hip_graph():
    model, size = model_for("dit", False)
    st = dict(guidance_scale=1.8, interval=(0.2, 0.7), solver="rk45", path_type="linear", mean_type="VELOCITY")
    args = sampler_args("flow", st, cpu_rng=False, sampler_type="ode", rtol=1e-3, atol=1e-4)
    diff = vaw_amd.FlowMatching(args=args, model_mean_type=vaw_amd.ModelMeanType.VELOCITY)
    torch.manual_seed(31)
    images, labels = vaw_amd.Sampler(args, torch.device(DEV), model, diff).sample(6, 3, size, 10)
    assert len(images) == len(labels) == 2
    cfg = vaw_amd.IntervalCFG(model, 10, 1.8, (0.2, 0.7), True).eval()
    torch.manual_seed(31)
    for b in range(2):
        y = torch.randint(0, 10, (3,), device=DEV)
        x = vaw_amd.flow_ode_sample(diff, cfg, torch.randn(3, 3, size, size, device=DEV), solver="rk45", rtol=1e-3, atol=1e-4, fused=False, y=y)
        ref = ops.finish_images(x).cpu().numpy()
        assert images[b].dtype.name == "uint8" and images[b].shape == (3, size, size, 3)
        assert (labels[b] == y.cpu().numpy()).all() and (images[b] == ref).all(), f"batch {b}: {int((images[b] != ref).sum())} bytes differ"
    assert images[0].tobytes() != images[1].tobytes()
    args = sampler_args("flow", st, cpu_rng=False, sampler_type="ode", hip_graph=True)
    with pytest.raises(ValueError, match="hip_graph.*rk45"):
        vaw_amd.Sampler(args, torch.device(DEV), model, diff).sample(6, 3, size, 10)

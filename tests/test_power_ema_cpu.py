"""Post-hoc EMA, the part that needs no GPU: the float64 host mathematics of vaw_amd/ema.py against the independent restatement
in power_ema_cases.py (which shares no code with the package), the refusals, the snapshot format and the C ABI of csrc/ema.hip."""
import os

import numpy as np
import pytest
import torch

import abi_cases
import power_ema_cases as cases
from conftest import REPO

import vaw_amd
from vaw_amd.ema import SNAPSHOT_FORMAT, PowerEMA, posthoc_ema

STEPS = list(range(256, 4097, 256))          # 16 snapshot times
DEFAULT = (0.05, 0.10)


def _entries():
    """(steps, sigma_rels) of the 32 stored averages in (step, sigma_rel) order"""
    return [t for t in STEPS for _ in DEFAULT], [s for _ in STEPS for s in DEFAULT]


@pytest.mark.parametrize("sigma_rel", [0.02, 0.05, 0.075, 0.10, 0.15, 0.25])
def test_sigma_rel_gamma_round_trip(sigma_rel):
    g = vaw_amd.sigma_rel_to_gamma(sigma_rel)
    assert g > -1 and abs(vaw_amd.gamma_to_sigma_rel(g) - sigma_rel) <= 1e-12
    assert abs(cases.sigma_rel_of(g) - sigma_rel) <= 1e-12 and abs(g - cases.gamma_of(sigma_rel)) <= 1e-9 * max(1.0, abs(g))


def test_the_two_default_exponents():
    assert abs(vaw_amd.sigma_rel_to_gamma(0.05) - 16.9722) < 5e-5 and abs(vaw_amd.sigma_rel_to_gamma(0.10) - 6.9372) < 5e-5


def test_closed_form_inner_product_is_the_quadrature():
    """<(300, 0.05), (1000, 0.10)>: midpoint rule with 3e6 points 1.35079345188e-6, closed form 1.35079345188e-6"""
    ga, gb = cases.gamma_of(0.05), cases.gamma_of(0.10)
    quad = cases.dot_quadrature(300.0, ga, 1000.0, gb, 3_000_000)
    for got in (vaw_amd.profile_dot(300, ga, 1000, gb), vaw_amd.profile_dot(1000, gb, 300, ga), cases.dot_closed(300.0, ga, 1000.0, gb)):
        print(f"closed form {got:.12e} quadrature {quad:.12e}")
        assert abs(got - quad) <= 1e-9 * quad
    assert abs(quad - 1.35079345188e-6) < 1e-16


@pytest.mark.parametrize("sigma_rel", DEFAULT)
def test_discrete_weights_sum_to_one_and_have_the_width(sigma_rel):
    """std of the tracked average's weights over theta_1 .. theta_T, in units of T, at T = 256: 0.049989 and 0.099995"""
    T = 256
    w = cases.discrete_weights(T, cases.gamma_of(sigma_rel))
    assert abs(w.sum() - 1.0) <= 1e-12
    j = np.arange(1, T + 1, dtype=np.float64) / T
    std = float(np.sqrt(np.sum(w * j * j) - np.sum(w * j) ** 2))
    print(f"sigma_rel {sigma_rel}: discrete std {std:.6f}")
    assert abs(std - sigma_rel) <= 3e-4 * sigma_rel
    # the package's c_t is the restatement's
    g = vaw_amd.sigma_rel_to_gamma(sigma_rel)
    for t in (1, 2, 3, 1000, 10 ** 6, 10 ** 7):
        assert abs(vaw_amd.power_ema_coefficient(t, g) - cases.coef(t, g)) <= 4 * np.spacing(cases.coef(t, g))
    assert vaw_amd.power_ema_coefficient(1, g) == 1.0


def test_coefficients_match_the_restatements_solve():
    """32 stored averages (16 times x the two default widths), targets between and outside them; cond(A) = 5.9e3"""
    steps, rels = _entries()
    gam = [cases.gamma_of(s) for s in rels]
    for t_out, s_out in ((4096, 0.075), (4096, 0.15), (3000, 0.03), (4096, 0.25)):
        take = [i for i, t in enumerate(steps) if t <= t_out]
        want, A = cases.solve([steps[i] for i in take], [gam[i] for i in take], t_out, cases.gamma_of(s_out))
        got = vaw_amd.posthoc_coefficients(steps, rels, t_out, s_out)
        print(f"target ({t_out}, {s_out}): cond(A) {np.linalg.cond(A):.3g}, max |difference| {np.abs(got[take] - want).max():.3g}")
        assert got.dtype == np.float64 and got.shape == (len(steps),)
        assert np.abs(got[take] - want).max() <= 1e-9 and abs(got.sum() - 1.0) <= 1e-12
        assert all(got[i] == 0.0 for i in range(len(steps)) if i not in take)


def test_a_tracked_profile_at_a_snapshot_time_is_its_unit_vector():
    steps, rels = _entries()
    for i in (0, 13, 31):
        got = vaw_amd.posthoc_coefficients(steps, rels, steps[i], rels[i])
        unit = np.zeros(len(steps))
        unit[i] = 1.0
        assert np.abs(got - unit).max() <= 1e-12, (i, np.abs(got - unit).max())


def test_end_to_end_in_float64():
    """A random walk tracked by the restatement, two widths that were never tracked reconstructed at T from the snapshots of the
    default two, against tracking them directly: error / max |direct - theta_T| 4.4e-4 (0.075) and 7.6e-4 (0.15)."""
    T = 4096
    theta = cases.random_walk(T, 64)
    steps, rels = _entries()
    kept = {s: cases.track(theta, cases.gamma_of(s), keep=set(STEPS))[1] for s in DEFAULT}
    for s_out in (0.075, 0.15):
        x = vaw_amd.posthoc_coefficients(steps, rels, T, s_out)
        recon = sum(c * kept[s][t] for c, t, s in zip(x, steps, rels))
        direct, _ = cases.track(theta, cases.gamma_of(s_out))
        err = np.abs(recon - direct).max() / np.abs(direct - theta[-1]).max()
        print(f"sigma_rel {s_out}: relative error {err:.3g}")
        assert err <= 2e-3


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -0.05, 0.2801, 0.3, float("nan"), float("inf"), "wide"])
def test_bad_sigma_rel_is_refused(bad):
    with pytest.raises(ValueError):
        vaw_amd.sigma_rel_to_gamma(bad)
    with pytest.raises(ValueError):
        vaw_amd.posthoc_coefficients([256], [0.05], 256, bad)
    with pytest.raises(ValueError):
        vaw_amd.posthoc_coefficients([256], [bad], 256, 0.05)
    with pytest.raises(ValueError):
        PowerEMA(cases.walk_module(8), (0.05, bad))


def test_bad_steps_duplicates_and_late_snapshots_are_refused():
    for steps in ([0, 256], [-1, 256], [1.5, 256], [True, 256]):
        with pytest.raises(ValueError):
            vaw_amd.posthoc_coefficients(steps, [0.05, 0.05], 512, 0.075)
    with pytest.raises(ValueError, match="duplicate"):
        vaw_amd.posthoc_coefficients([256, 512, 256], [0.05, 0.05, 0.05], 512, 0.075)
    with pytest.raises(ValueError, match="at or before"):
        vaw_amd.posthoc_coefficients([256, 512], [0.05, 0.10], 255, 0.075)
    with pytest.raises(ValueError):
        vaw_amd.posthoc_coefficients([256, 512], [0.05], 512, 0.075)
    assert vaw_amd.posthoc_coefficients([256, 512], [0.05, 0.10], 256, 0.05).tolist() == [1.0, 0.0]


def test_power_ema_construction_refusals():
    with pytest.raises(ValueError):                                          # K = 5
        PowerEMA(cases.walk_module(8), (0.05, 0.06, 0.07, 0.08, 0.09))
    with pytest.raises(ValueError):
        PowerEMA(cases.walk_module(8), ())
    with pytest.raises(ValueError):
        PowerEMA(cases.walk_module(8), (0.05, 0.05))
    for exc in (ValueError, TypeError):                                      # a non-FlatModule: both, as FusedAdamW says TypeError
        with pytest.raises(exc):
            PowerEMA(torch.nn.Linear(4, 4))
    m = cases.walk_module(8)
    m.register_buffer("running", torch.zeros(3))
    with pytest.raises(ValueError, match="buffers"):
        PowerEMA(m)


def test_no_cpu_fallback():
    pe = PowerEMA(cases.walk_module(8))
    with pytest.raises(vaw_amd.VawError):
        pe.update()


def _snapshot(width, step, extra=0):
    s = PowerEMA(cases.walk_module(width, extra)).snapshot()
    s["step"] = step
    for k, f in enumerate(s["flat"]):
        f.copy_(torch.arange(f.numel(), dtype=torch.float32) * (k + 1))
    return s


def test_mixed_layouts_and_foreign_dicts_are_refused():
    with pytest.raises(ValueError, match="layout"):
        posthoc_ema([_snapshot(100, 256), _snapshot(100, 512, extra=5)], 0.075)
    with pytest.raises(ValueError, match="layout"):
        posthoc_ema([_snapshot(100, 256), _snapshot(200, 512)], 0.075)
    with pytest.raises(ValueError):
        posthoc_ema([{"step": 3}], 0.075)
    with pytest.raises(ValueError):
        posthoc_ema([], 0.075)
    with pytest.raises(ValueError, match="at or before"):
        posthoc_ema([_snapshot(100, 256), _snapshot(100, 512)], 0.075, step=100)
    with pytest.raises(ValueError, match="layout"):
        posthoc_ema([_snapshot(100, 256)], 0.075, into=cases.walk_module(200))
    pe = PowerEMA(cases.walk_module(100))
    with pytest.raises(ValueError, match="layout"):
        pe.load_state_dict(_snapshot(200, 256))
    with pytest.raises(ValueError):
        PowerEMA(cases.walk_module(100), (0.05, 0.15)).load_state_dict(_snapshot(100, 256))
    with pytest.raises(ValueError, match="layout"):
        pe.copy_to(cases.walk_module(200), 0.05)
    with pytest.raises(ValueError, match="not tracked"):
        pe.copy_to(cases.walk_module(100), 0.075)


def test_snapshot_survives_weights_only_serialisation(tmp_path):
    snap = _snapshot(100, 768)
    assert set(snap) == {"format", "step", "sigma_rels", "layout", "flat"} and snap["format"] == SNAPSHOT_FORMAT
    assert snap["sigma_rels"] == [0.05, 0.10] and snap["layout"] == {"theta": (0, 100, False)}
    assert [f.dtype for f in snap["flat"]] == [torch.float32] * 2 and all(f.device.type == "cpu" and f.numel() == 128 for f in snap["flat"])
    path = os.path.join(tmp_path, "snap.pt")
    torch.save(snap, path)
    back = torch.load(path, weights_only=True)
    assert {k: v for k, v in back.items() if k != "flat"} == {k: v for k, v in snap.items() if k != "flat"}
    assert all(torch.equal(a, b) for a, b in zip(back["flat"], snap["flat"]))
    pe = PowerEMA(cases.walk_module(100))
    pe.load_state_dict(back)                                                  # the state of a PowerEMA is its snapshot
    again = pe.state_dict()
    assert again["step"] == 768 and all(torch.equal(a, b) for a, b in zip(again["flat"], snap["flat"]))


# ---- the native side, as far as it shows without a GPU ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vaw_ema_profiles_coef", "vaw_ema_profiles_update", "vaw_lincomb_accum_f64", "vaw_f64_to_f32"])
def test_abi(name):
    abi_cases.assert_bound_as_declared(vaw_amd.lib(), name)


def test_ema_hip_is_built_without_contraction():
    mk = open(os.path.join(REPO, "variance-aware-weight_amd", "csrc", "Makefile")).read()
    assert " ema.hip " in mk and "EXTRA_ema = -ffp-contract=off" in mk


def test_checkpoint_keyword_is_trailing_and_optional():
    import inspect
    sig = inspect.signature(vaw_amd.save_checkpoint).parameters, inspect.signature(vaw_amd.load_checkpoint).parameters
    assert all(list(p)[-1] == "power_ema" and p["power_ema"].default is None for p in sig)
    assert vaw_amd._lib.EMA_MAX_PROFILES == 4

"""The per-tensor criterion of tests/model_grad_cases.py, shown on the CPU (oracle only) to tell rounding from a wiring error at
every case: the float64 reference is the oracle and nothing else, no tensor is exempt, every bound stays below half of the mildest
mutation, every mutation is rejected, and correct bf16 / fp8 / f32 arithmetic is accepted.  tests/test_gpu_model_grads.py holds
the HIP models to the same function."""
import pytest
import torch

import model_grad_cases as C


@pytest.fixture(params=C.CASES, ids=C.CASE_IDS)
def case(request):
    return request.param


def test_float64_patch_changes_nothing_else(case):
    """The float64 run lifts the oracle's internal f32 casts (timestep embedding, GroupNorm32, UNet softmax).  It agrees with the
    plain f32 oracle run to 1e-5 relative L2 at the output, the input gradient and every parameter gradient."""
    g64, g32 = C.reference(case), C.reference_f32(case)
    assert set(g64) == set(g32) and C.OUT in g64 and C.GX in g64
    assert all(v.dtype == torch.float64 for v in g64.values())
    err = C.errors(g32, g64)
    assert max(err.values()) <= 1e-5, max(err.items(), key=lambda kv: kv[1])


def test_no_tensor_is_exempt(case):
    """Every trainable tensor has a float64 gradient whose rms is above 1e-4 of the model's overall gradient rms (a UNet with one
    channel per GroupNorm group, or a model left at its zero initialisation, would not), and a yardstick above zero."""
    g64 = C.reference(case)
    om = C.build_oracle(case)
    trainable = {k for k, p in om.named_parameters() if p.requires_grad}
    assert trainable | {C.OUT, C.GX} == set(g64)
    frac = C.rms_fractions(g64)
    k = min(frac, key=frac.get)
    assert frac[k] > C.MIN_RMS_FRACTION, (k, frac[k])
    _, e_ref = C.case_yardstick(case)
    assert all(0.0 < e < 1.0 for e in e_ref.values())


def test_cap_and_every_mutation_rejected(case):
    """Cap: margin_k * e_ref[k] < half of the smallest mutation error at k, for every tensor a mutation touches (bf16 cases: every
    tensor, through the 7/8 scale).  And the criterion rejects every mutation, at a tensor the mutation touched."""
    g64 = C.reference(case)
    _, e_ref = C.case_yardstick(case)
    bound = C.bounds(case, e_ref)
    small = C.smallest_mutation_error(case, g64)
    if case.mode == "bf16":
        assert set(small) == set(g64)
    slack = {k: bound[k] / (C.CAP_FRACTION * e) for k, (e, _) in small.items()}
    k = max(slack, key=slack.get)
    kb, km = max(bound, key=bound.get), min(small, key=lambda q: small[q][0])
    print(f"\n{case.id}: largest bound {bound[kb]:.4f} ({kb}); smallest mutation error {small[km][0]:.4f} ({small[km][1]}); "
          f"tightest cap: bound {bound[k]:.4f} vs half of {small[k][0]:.4f} at {k}")
    assert slack[k] < 1.0, (k, bound[k], small[k])
    for _pat, m, reason in case.margins:
        assert m > C.MARGIN and len(reason) > 20
    muts = C.mutations(case, g64)
    names = {n for n, _, _ in muts}
    want = set(C.MUTATIONS) - {"unet_skip_out"} - ({"unet_qkv_order", "unet_doubled"} if case.family == "dit" else {"qk_swap", "head_swap", "adaln_chunk"})
    assert names == want
    for name, label, changed in muts:
        assert all(not torch.equal(v, g64[k]) for k, v in changed.items())
        fails, _ = C.criterion(case, C.mutate(g64, changed), g64, e_ref)
        assert {k for k, _, _ in fails} == set(changed), (name, label, fails)
    if case.family == "unet":        # the one listed mutation that is no error (see _m_unet_skip_out)
        a, b = C.SKIP_OUT_PAIRS
        assert g64[a].shape == g64[b].shape and C.rel_err(g64[a], g64[b]) < 1e-12
        assert not [k for k in g64 if k.endswith("skip_connection.weight") and g64[k].shape == g64[k.replace("skip_connection", "out_layers.3")].shape]


def test_correct_arithmetic_is_accepted(case):
    """The criterion accepts the yardstick's own gradients (bf16 autocast; fp8 cases: the fake-quantised oracle AND plain bf16
    autocast, which is more accurate) and the f32 oracle's; a dict that lacks a tensor fails."""
    g64 = C.reference(case)
    g_ref, e_ref = C.case_yardstick(case)
    for got in (g_ref, C.reference_f32(case)) + ((C.yardstick(case)[0],) if case.mode == "fp8" else ()):
        fails, worst = C.criterion(case, got, g64, e_ref)
        assert not fails and worst[0] <= C.MARGIN, (fails[:3], worst)
    k = next(iter(g64))
    fails, _ = C.criterion(case, {q: v for q, v in g64.items() if q != k}, g64, e_ref)
    assert [f[0] for f in fails] == [k]


def test_fp8_yardstick_follows_the_gradient_format():
    """e5m2 carries one mantissa bit less than e4m3: the weight gradients of the fake-quantised Linear layers move with the
    format, the forward (e4m3 either way) does not."""
    a, b = C.BY_ID["dit_fp8_jit_e5m2"], C.BY_ID["dit_fp8_jit_e4m3"]
    (ga, ea), (gb, eb) = C.case_yardstick(a), C.case_yardstick(b)
    assert torch.equal(ga[C.OUT], gb[C.OUT])
    k = "blocks.0.mlp.fc1.weight"
    assert ea[k] > eb[k] > 3 * C.yardstick(a)[1][k]


def test_key_sets_of_oracle_and_hip_models_agree(case):
    vaw_amd = pytest.importorskip("vaw_amd")
    om = C.build_oracle(case)
    hm = (vaw_amd.DiT if case.family == "dit" else vaw_amd.UNetModel)(**case.kwargs)
    o, h = dict(om.named_parameters()), dict(hm.named_parameters())
    assert set(o) == set(h)
    assert all(o[k].shape == h[k].shape and o[k].requires_grad == h[k].requires_grad for k in o)

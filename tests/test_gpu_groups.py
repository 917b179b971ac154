"""The grouped launches' plumbing over a long run: the pinned staging of vaw_upload_table is a bounded pool that never hands a buffer
out before its copy has completed, the group caches (ops.GroupCache) keep alternating row counts resident and stay within their
bound, and a backward that raised leaves nothing queued for the next step.  Run on the MI355X box: pytest -m gpu."""
import ctypes

import pytest
import torch

from conftest import perturb_

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd._lib import BF16, lib, ptr

DEV = "cuda"


def _buffers():
    """pinned staging buffers vaw_upload_table has allocated so far (process-wide)"""
    n, nbytes, cap = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    lib().vaw_debug_upload_table_stats(ctypes.byref(n), ctypes.byref(nbytes), ctypes.byref(cap))
    assert n.value >= cap.value >= 0 and nbytes.value >= 4096 * n.value
    return n.value


def _reduce_case(seed):
    """two folds, (R = 3, N = 40) and (R = 5, N = 33: past the 32-column block edge) -> (parts, outs, ReduceGroup)"""
    g = torch.Generator().manual_seed(seed)
    parts = [(torch.randn(R, N, generator=g) * 3).to(DEV) for R, N in ((3, 40), (5, 33))]
    outs = [torch.full((p.shape[1],), float("nan"), device=DEV) for p in parts]
    return parts, outs, ops.ReduceGroup([(ptr(p), ptr(o), p.shape[0], p.shape[1]) for p, o in zip(parts, outs)], torch.device(DEV))


def _wgrad_case(seed, M=16, N=24, K=64):
    g = torch.Generator().manual_seed(seed)
    dy, x = torch.randn(K, M, generator=g).to(DEV).bfloat16(), torch.randn(K, N, generator=g).to(DEV).bfloat16()
    dw = torch.full((M, N), float("nan"), device=DEV)
    return (dy, x), dw, ops.WgradGroup([(ptr(dy), ptr(x), ptr(dw), M, N, M, N, N)], K, torch.device(DEV))


def test_upload_pool_is_bounded_over_many_groups():
    """200 groups built and launched one after another, each finished before the next: one staging buffer serves them all, and
    every fold is bitwise vaw_reduce_rows' (the header's promise: the same summation tree)."""
    torch.cuda.synchronize()
    before = _buffers()
    for i in range(200):
        parts, outs, grp = _reduce_case(i)
        grp.launch(0.0)
        torch.cuda.synchronize()
        for p, o in zip(parts, outs):
            ref = torch.empty_like(o)
            ops.reduce_rows(ptr(p), p.shape[0], p.shape[1], ptr(ref), 0.0)
            assert torch.equal(o, ref), i
    assert _buffers() - before <= 1, (before, _buffers())


def test_upload_pool_hands_no_buffer_out_early():
    """64 + 64 groups with distinct data launched back to back with no synchronisation: had a staging buffer been reused before its
    copy completed, some group would have run on another group's table.  Each output against the same group launched alone."""
    red = [_reduce_case(1000 + i) for i in range(64)]
    wg = [_wgrad_case(2000 + i) for i in range(64)]
    torch.cuda.synchronize()
    for (_, _, rg), (_, _, g) in zip(red, wg):
        rg.launch(0.0)
        g.launch(BF16, 0.0)
    torch.cuda.synchronize()
    for i, ((parts, outs, _), ((dy, x), dw, _)) in enumerate(zip(red, wg)):
        got = [o.clone() for o in outs] + [dw.clone()]
        alone_r = ops.ReduceGroup([(ptr(p), ptr(o), p.shape[0], p.shape[1]) for p, o in zip(parts, outs)], torch.device(DEV))
        alone_w = ops.WgradGroup([(ptr(dy), ptr(x), ptr(dw), 16, 24, 16, 24, 24)], 64, torch.device(DEV))
        for o in outs + [dw]:
            o.fill_(float("nan"))
        alone_r.launch(0.0)
        alone_w.launch(BF16, 0.0)
        torch.cuda.synchronize()
        for a, b in zip(got, outs + [dw]):
            assert torch.isfinite(b).all() and torch.equal(a, b), i
    # distinct data did give distinct results: equality above is no accident of equal tables
    assert not torch.equal(wg[0][1], wg[1][1]) and not torch.equal(red[0][1][0], red[1][1][0])


def test_dit_alternating_row_counts_hit_two_resident_folds():
    """The fold's row counts move with the GEMM kernel the producers ran on (here vaw_debug_gemm_tile: 128-row tiles against the
    64-row ring; in training, the CUs reserved on the synchronising backward of a gradient accumulation).  Alternating them must
    cost two groups and two uploads in all, not one of each per backward."""
    torch.manual_seed(5)
    m = vaw_amd.DiT(image_size=32, patch_size=2, in_channels=4, hidden_size=256, depth=2, num_heads=4, num_classes=10,
                    class_dropout_prob=0.0, learn_sigma=False, compute_dtype="bf16").to(DEV).train()
    perturb_(m, 3, 0.05)
    m.ensure_flat()
    assert m.defer_wgrad
    g = torch.Generator().manual_seed(9)
    x = torch.randn(16, 4, 32, 32, generator=g).to(DEV)           # 16 x 256 tokens = 4096 rows
    t = (torch.rand(16, generator=g) * 999).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    gout = torch.randn(16, 4, 32, 32, generator=g).to(DEV)
    grads, misses, bufs = [], [], []
    try:
        for i in range(6):
            lib().vaw_debug_gemm_tile(0 if i % 2 == 0 else 6)
            m.zero_grad_flat()
            out, _ = m(x, t, y)
            (out * gout).sum().backward()
            torch.cuda.synchronize()
            grads.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
            misses.append(m._ws_cur.bias_groups.misses)
            bufs.append(_buffers())
    finally:
        lib().vaw_debug_gemm_tile(-1)
    cache = m._ws_cur.bias_groups
    rows = [k[4] for k in cache]
    assert len(rows) == 2 and rows[0] != rows[1] and {k[:4] for k in cache} == {(0, 1, m._gbase, True)}, list(cache)
    print(f"\nrow counts of the two folds: {rows[0]} / {rows[1]}; misses per pass {misses}; staging buffers per pass {bufs}")
    assert misses[1:] == [2] * 5 and cache.hits == 4, (misses, cache.hits)
    assert bufs[1:] == [bufs[1]] * 5, bufs
    assert len(m._ws_cur.wgrad_groups) == 1 and m._ws_cur.wgrad_groups.misses == 1
    for i in (2, 3, 4, 5):
        assert grads[i].keys() == grads[i - 2].keys() and len(grads[i]) > 20
        assert [k for k in grads[i] if not torch.equal(grads[i][k], grads[i - 2][k])] == [], i


def _tiny_unet():
    torch.manual_seed(42)
    m = vaw_amd.UNetModel(16, 3, 32, 3, 1, attention_resolutions=(1, 2), channel_mult=(1, 2), num_heads=2, use_scale_shift_norm=True,
                          resblock_updown=True, use_new_attention_order=True, compute_dtype="bf16").to(DEV).train()
    perturb_(m, 5)
    m.ensure_flat()
    m._grouped_wgrad = True
    return m


def _unet_inputs(seed, B=8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, 16, 16, generator=g).to(DEV), torch.randint(0, 1000, (B,), generator=g).to(DEV),
            torch.randn(B, 3, 16, 16, generator=g).to(DEV))


def _unet_step(m, inp):
    x, t, gout = inp
    m.zero_grad_flat()
    (m(x, t) * gout).sum().backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_unet_interrupted_backward_does_not_leak_into_the_next_step(monkeypatch):
    """A backward that raises part-way leaves deferred (dy, x, dW) entries queued; the next step must not launch them."""
    class Boom(Exception):
        pass

    hit, clean = _tiny_unet(), _tiny_unet()
    assert torch.equal(hit._flat, clean._flat)
    colsum = ops.colsum

    def raising(*a, **kw):          # the bias-gradient pass of the second 1 x 1 layer whose weight gradient was queued
        if sum(len(v) for v in hit._pend_wgrad.values()) >= 2:
            raise Boom()
        return colsum(*a, **kw)

    xa, ta, ga = _unet_inputs(1)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "colsum", raising)
        with pytest.raises(Boom):
            (hit(xa, ta) * ga).sum().backward()
    torch.cuda.synchronize()
    assert ops.colsum is colsum and sum(len(v) for v in hit._pend_wgrad.values()) >= 2      # step A did leave entries queued
    inp = _unet_inputs(2)
    got, ref = _unet_step(hit, inp), _unet_step(clean, inp)
    assert not hit._pend_wgrad and bool(hit._wgrad_groups) and bool(clean._wgrad_groups)
    assert got.keys() == ref.keys() and len(ref) > 20
    assert [k for k in ref if not torch.equal(got[k], ref[k])] == []


def test_unet_group_cache_and_staging_stay_bounded_under_address_churn(record_property):
    """Every step builds its groups anew (the cache is emptied before it, as if every activation address had moved): the cache
    stays within its bound and the staging pool stops growing once a step's uploads have been seen."""
    m, inp = _tiny_unet(), _unet_inputs(3)
    bufs = []
    for _ in range(6):
        m._wgrad_groups.clear()
        _unet_step(m, inp)
        assert 0 < len(m._wgrad_groups) <= m._wgrad_groups.bound == 64
        bufs.append(_buffers())
    assert bufs[5] == bufs[1], bufs
    # ordinary steps at fixed shapes: how often the cache misses is up to torch's allocator (whether activations come back at the
    # addresses of the step before), so the figure is reported, not asserted
    m2 = _tiny_unet()
    for _ in range(6):
        _unet_step(m2, inp)
        assert len(m2._wgrad_groups) <= 64
    c = m2._wgrad_groups
    print(f"\nsix ordinary steps: {c.misses} misses, {c.hits} hits, {len(c)} groups resident; staging buffers {bufs}")
    record_property("unet_group_cache_misses_6_steps", c.misses)

"""The attention kernels (csrc/attention.hip, attention_mfma.hip, attention_bwd_big.hip) against a float64 statement of
softmax(scale q k^T) v on the exact inputs, through their C entry points, over every launch the plan (vaw_attn_plan) can make: each
kernel variant at each head-width image it instantiates, padded head dims, the production shapes of the model zoo, all four layouts,
misaligned operands, and input regimes that force the online softmax's branches (peaked rows, a maximum that first appears in the
last key block by less and by more than the lazy-rescale threshold, logits past exp's f32 range, exactly uniform rows).

Errors are judged element by element against a bound computed in float64 from the same expressions taken in absolute values:
  o:      c u (P |V|) + u |o|
  dV:     c u (P^T |dO|) + u |dV|
  dQ, dK: c u scale (P o (|dO| |V|^T + |delta|)) |K|  (transposed, with |Q|, for dK) + u |dQ|, |dK|
  lse:    2^-16 (1 + max_j |s_ij|)
u = 2^-8 for bf16 storage; for f32 (the rowwise kernels) u = 2^-24 (T + hd (1 + max |s|)): a length-T sum, and a length-hd dot
product whose absolute error __expf turns into a relative one.  One c per dtype, the same for every shape and variant.  Every case
records its worst err / bound (record_property), so a run with --junitxml gives each variant's margin.

Each backward runs twice: chained after its own forward, and from the reference o (rounded to the act dtype) and lse (rounded to
f32), so a forward error can neither hide nor fake a backward one."""
import math
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops
from vaw_amd._lib import BF16, F32, ptr

DEV = "cuda"
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
C_BOUND = {BF16: 1.0, F32: 1.0}
SWITCHES = ("VAW_ATTN_FWD_BIG", "VAW_ATTN_BWD_BIG", "VAW_ATTN_QG2", "VAW_ATTN_BWD_G2")
CANARY = 12345.5
REGIMES_ALL = ("flat", "peaked", "late", "large", "uniform")


def _u(dt, T, hd, smax):
    return 2.0 ** -8 if dt == BF16 else 2.0 ** -24 * (T + hd * (1 + smax))


# name -> (B, H, T, hd, dt, layout, switches, regimes); layout "token" | "nhwc_new" | "nhwc_legacy" | "channel", "+off": q / k / v
# one element and dq / dk / dv 2 bytes past an aligned base
CASES = {
    # rowwise f32
    "r32_t100_hd40": (3, 2, 100, 40, F32, "token", {}, ("flat", "peaked", "large")),
    "r32_t1": (2, 2, 1, 16, F32, "token", {}, ("flat", "uniform")),
    "r32_channel": (2, 3, 64, 32, F32, "channel", {}, ("flat", "peaked", "late")),
    "r32_legacy_t17": (1, 2, 17, 72, F32, "nhwc_legacy", {}, ("flat", "peaked")),
    "r32_t1024": (1, 1, 1024, 64, F32, "nhwc_new", {}, REGIMES_ALL),
    # rowwise bf16: T off the 64 grid, channel-major, misaligned operands, T = 1
    "r16_t100_hd72": (2, 2, 100, 72, BF16, "token", {}, ("flat", "peaked", "late")),
    "r16_off": (1, 2, 128, 64, BF16, "token+off", {}, ("flat", "peaked")),
    "r16_off_nhwc": (1, 2, 256, 72, BF16, "nhwc_new+off", {}, ("flat", "peaked")),
    "r16_channel": (1, 2, 128, 24, BF16, "channel", {}, ("flat", "peaked")),
    "r16_t1": (1, 3, 1, 8, BF16, "token", {}, ("flat",)),
    # production shapes (batch 1 .. 3), all regimes
    "dit_b4": (2, 12, 64, 64, BF16, "token", {}, REGIMES_ALL),
    "dit_xl2": (1, 16, 256, 72, BF16, "token", {}, REGIMES_ALL),
    "unet64_t256": (1, 4, 256, 96, BF16, "nhwc_new", {}, REGIMES_ALL),
    "unet64_t64": (2, 4, 64, 96, BF16, "nhwc_new", {}, REGIMES_ALL),
    "adm_t1024": (1, 2, 1024, 64, BF16, "nhwc_new", {}, REGIMES_ALL),
    "adm_t256": (2, 2, 256, 64, BF16, "nhwc_new", {}, REGIMES_ALL),
    "unet32_t64": (3, 4, 64, 64, BF16, "nhwc_new", {}, REGIMES_ALL),
    "unet32_t16": (2, 4, 16, 64, BF16, "nhwc_new", {}, REGIMES_ALL),
    "adm32_t256": (1, 4, 256, 32, BF16, "nhwc_new", {}, REGIMES_ALL),
    "adm32_t64": (2, 4, 64, 32, BF16, "nhwc_new", {}, REGIMES_ALL),
    "ldm_t1024": (1, 4, 1024, 32, BF16, "nhwc_new", {}, REGIMES_ALL),
    "ldm_t256": (1, 4, 256, 32, BF16, "nhwc_new", {}, REGIMES_ALL),
    # legacy channel order on the MFMA kernels
    "legacy_t256_hd64": (2, 2, 256, 64, BF16, "nhwc_legacy", {}, ("flat", "peaked", "late")),
    "legacy_t256_hd96": (1, 2, 256, 96, BF16, "nhwc_legacy", {}, ("flat", "peaked", "late")),
    "legacy_t192_hd32": (1, 2, 192, 32, BF16, "nhwc_legacy", {}, ("flat", "peaked")),
    # every image of the T64 / G1 kernels, padded head dims
    "t64_hd24": (2, 2, 64, 24, BF16, "token", {}, ("flat", "peaked")),
    "t64_hd120": (2, 2, 64, 120, BF16, "token", {}, ("flat", "peaked", "large")),
    "t192_hd16": (1, 2, 192, 16, BF16, "token", {}, ("flat", "peaked", "late")),
    "t192_hd40": (1, 2, 192, 40, BF16, "token", {}, ("flat", "peaked", "late")),
    "t192_hd96": (1, 2, 192, 96, BF16, "token", {}, ("flat", "peaked", "late")),
    "t192_hd128": (1, 2, 192, 128, BF16, "token", {}, ("flat", "peaked", "late")),
    "t256_hd104": (1, 2, 256, 104, BF16, "token", {}, ("flat", "peaked", "late")),
    "t320_hd24": (1, 3, 320, 24, BF16, "token", {}, ("flat", "peaked", "late")),
    "t128_hd8": (2, 2, 128, 8, BF16, "token", {}, ("flat", "peaked")),
    # the switches: the other forward / backward forms
    "fwdbig64": (1, 2, 256, 40, BF16, "token", {"VAW_ATTN_FWD_BIG": "1"}, ("flat", "peaked", "late", "large")),
    "fwdbig64_nt4": (1, 2, 512, 64, BF16, "token", {"VAW_ATTN_FWD_BIG": "1", "VAW_ATTN_BWD_BIG": "1"}, ("flat", "peaked", "late")),
    "g1_qg2off": (1, 2, 256, 64, BF16, "token", {"VAW_ATTN_QG2": "0", "VAW_ATTN_BWD_BIG": "0"}, ("flat", "peaked", "late")),
    "g1_qg2off_hd72": (1, 2, 256, 72, BF16, "token", {"VAW_ATTN_QG2": "0", "VAW_ATTN_FWD_BIG": "0", "VAW_ATTN_BWD_BIG": "0"},
                       ("flat", "peaked", "late", "large")),
    "g2_hd96": (1, 2, 128, 96, BF16, "token", {"VAW_ATTN_FWD_BIG": "0", "VAW_ATTN_BWD_BIG": "0", "VAW_ATTN_BWD_G2": "0"},
                ("flat", "peaked", "late")),
    "nt4_hd72": (1, 2, 256, 72, BF16, "token", {"VAW_ATTN_BWD_BIG": "1"}, ("flat", "peaked", "late", "large")),
    "nt4_hd96": (1, 2, 512, 96, BF16, "nhwc_new", {"VAW_ATTN_BWD_BIG": "1"}, ("flat", "peaked", "late")),
}
PARAMS = [(name, regime) for name, c in CASES.items() for regime in c[7]]


class _env:
    """the case's attention switches (vaw_attn_plan reads them on every call); the others unset"""

    def __init__(self, sw):
        self.sw = sw

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.sw)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _layout(B, H, T, hd, layout):
    """(desc, k offset, v offset, element offset of q and dq, o buffer size, qkv buffer size), offsets and sizes in elements"""
    base = layout.split("+")[0]
    off = 1 if layout.endswith("+off") else 0
    D = H * hd
    if base == "token":
        desc, ko, vo = ops.attn_desc_token_major(B, H, T, hd), D, 2 * D
    elif base == "channel":
        desc, ko, vo = ops.attn_desc_channel_major(B, H, T, hd), D * T, 2 * D * T
    else:
        desc, ko, vo = ops.attn_desc_nhwc(B, H, T, hd, base == "nhwc_new")
    return desc, ko, vo, off, B * T * D, 3 * B * T * D


def _view(buf, desc, start, o=False):
    """[B, H, T, hd] strided view of a flat buffer from element `start` (q / k / v strides, or the o strides)"""
    st = (desc.o_sb, desc.o_sh, desc.o_st, desc.o_sd) if o else (desc.q_sb, desc.q_sh, desc.q_st, desc.q_sd)
    return buf.as_strided((desc.B, desc.H, desc.T, desc.hd), st, buf.storage_offset() + start)


def _inputs(B, H, T, hd, regime, tdt, seed):
    """q, k, v, dO [B, H, T, hd] as float64 holding act-dtype values"""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(B, H, T, hd, generator=g, dtype=torch.float64)
    scale = hd ** -0.5
    q, k, v, do = r() * 0.7, r() * 0.7, r() * 0.7, r()
    if regime == "peaked":                   # logits with std ~ 6: most rows nearly one-hot
        q, k = q * 3.5, k * 3.5
    elif regime == "large":                  # logits of magnitude 40 .. 100 (f32 exp overflows past 88.7); o far from 0
        q, k, v = q * 7, k * 7, v + 4
    elif regime == "uniform":                # all keys of a head equal: P exactly uniform
        k = k[:, :, :1].expand(B, H, T, hd).clone()
    q, k, v, do = (t.to(tdt).double() for t in (q, k, v, do))
    if regime == "late" and T > 64:
        # channels 0 / 1 of k are zero except at key jl (the last one, in the last 64-key block) / jf (in the first block); q's
        # channels 0 / 1 carry per-row boosts of those two keys.  Rows i % 3 == 0 get their maximum at jl, 3 log2 units above the
        # maximum of the blocks before (the lazy branch: p up to 8), rows i % 3 == 1 40 units above (the rescale branch), rows
        # i % 3 == 2 keep theirs at jf in the first block.
        jl, jf = T - 1, 5
        k[..., :2] = 0
        k[:, :, jl, 0] = 1.0
        k[:, :, jf, 1] = 1.0
        q[..., :2] = 0
        s = (q @ k.transpose(-1, -2)) * scale
        m_early = s[..., :T - 64].amax(-1)
        excess = torch.tensor([3.0, 40.0, 0.0] * ((T + 2) // 3), dtype=torch.float64)[:T] * math.log(2)
        keep = torch.arange(T) % 3 == 2
        b_last = torch.where(keep, torch.full_like(m_early, -30.0), m_early + excess - s[..., jl])
        b_first = torch.where(keep, torch.full_like(m_early, 15.0), torch.zeros_like(m_early))
        q[..., 0] = (b_last / scale).to(tdt).double()
        q[..., 1] = (b_first / scale).to(tdt).double()
    return q, k, v, do


def _reference(q, k, v, do, scale):
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (qr @ kr.transpose(-1, -2)) * scale
    p = torch.softmax(s, -1)
    o = p @ vr
    dq, dk, dv = torch.autograd.grad(o, (qr, kr, vr), do)
    s, p, o = s.detach(), p.detach(), o.detach()
    return dict(s=s, p=p, o=o, lse=torch.logsumexp(s, -1), dq=dq, dk=dk, dv=dv, delta=(do * o).sum(-1, keepdim=True))


def _bounds(ref, q, k, v, do, scale, u, c):
    p = ref["p"]
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    w = p * (ado @ av.transpose(-1, -2) + ref["delta"].abs())
    return dict(o=c * u * (p @ av) + u * ref["o"].abs(),
                dv=c * u * (p.transpose(-1, -2) @ ado) + u * ref["dv"].abs(),
                dq=c * u * scale * (w @ ak) + u * ref["dq"].abs(),
                dk=c * u * scale * (w.transpose(-1, -2) @ aq) + u * ref["dk"].abs(),
                lse=2.0 ** -16 * (1 + ref["s"].abs().amax(-1)))


def _ratio(got, want, bound):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - want).abs() / bound.clamp_min(1e-300)).max())


def _addrs(base_ptr, off, ko, vo, es):
    a = base_ptr + es * off
    return a, a + es * ko, a + es * vo


def _case_plans(name):
    """the (direction, variant, hd_image) the case runs, asked of the plan at the case's alignment"""
    B, H, T, hd, dt, layout, sw, _ = CASES[name]
    desc, ko, vo, off, _, _ = _layout(B, H, T, hd, layout)
    es = 4 if dt == F32 else 2
    q, g = _addrs(1 << 20, off, ko, vo, es), _addrs(1 << 24, off, ko, vo, es)
    with _env(sw):
        f = ops.attn_plan(L.ATTN_FWD, dt, desc, *q, 1 << 28)
        b = ops.attn_plan(L.ATTN_BWD, dt, desc, *q, 1 << 28, *g)
    return (L.ATTN_FWD, f.variant, f.hd_image), (L.ATTN_BWD, b.variant, b.hd_image)


@pytest.mark.parametrize("name,regime", PARAMS)
def test_attention_parity(name, regime, record_property):
    B, H, T, hd, dt, layout, sw, _ = CASES[name]
    tdt, es = TORCH_DT[dt], (4 if dt == F32 else 2)
    scale = hd ** -0.5
    desc, ko, vo, off, osize, qsize = _layout(B, H, T, hd, layout)
    q, k, v, do = _inputs(B, H, T, hd, regime, tdt, seed=zlib.crc32(f"{name}/{regime}".encode()))
    ref = _reference(q, k, v, do, scale)
    bnd = _bounds(ref, q, k, v, do, scale, _u(dt, T, hd, float(ref["s"].abs().max())), C_BOUND[dt])
    # device buffers in the case's layout: k / v at their offsets from q, o / dO with the o strides
    qkv_h = torch.zeros(qsize + off, dtype=tdt)
    for t, start in ((q, off), (k, off + ko), (v, off + vo)):
        _view(qkv_h, desc, start).copy_(t.to(tdt))
    do_h = torch.zeros(osize, dtype=tdt)
    _view(do_h, desc, 0, o=True).copy_(do.to(tdt))
    o_iso_h = torch.zeros(osize, dtype=tdt)
    _view(o_iso_h, desc, 0, o=True).copy_(ref["o"].to(tdt))
    qkv, dO, o_iso = qkv_h.to(DEV), do_h.to(DEV), o_iso_h.to(DEV)
    lse_iso = ref["lse"].float().reshape(-1).to(DEV)
    o = torch.full((osize,), CANARY, device=DEV, dtype=tdt)
    lse = torch.full((B * H * T,), CANARY, device=DEV)
    delta = torch.empty(B * H * T, device=DEV)
    fplan, bplan = _case_plans(name)
    a = _addrs(ptr(qkv), off, ko, vo, es)
    ratios = {}
    with _env(sw):
        p = ops.attn_plan(L.ATTN_FWD, dt, desc, *a, ptr(o))
        assert (L.ATTN_FWD, p.variant, p.hd_image) == fplan
        ops.attn_fwd(dt, desc, *a, ptr(o), ptr(lse))
        o2, lse2 = torch.empty_like(o), torch.empty_like(lse)
        ops.attn_fwd(dt, desc, *a, ptr(o2), ptr(lse2))
        ratios["o"] = _ratio(_view(o.cpu(), desc, 0, o=True), ref["o"], bnd["o"])
        ratios["lse"] = _ratio(lse.cpu().view(B, H, T), ref["lse"], bnd["lse"])
        assert torch.equal(o, o2) and torch.equal(lse, lse2), "forward not deterministic"
        # backward chained (the kernel's o / lse) and isolated (reference o in the act dtype, reference lse in f32)
        for mode, (oo, ll) in (("chained", (o, lse)), ("isolated", (o_iso, lse_iso))):
            dqkv = torch.full((qsize + off,), CANARY, device=DEV, dtype=tdt)
            g = _addrs(ptr(dqkv), off, ko, vo, es)
            bp = ops.attn_plan(L.ATTN_BWD, dt, desc, *a, ptr(dO), *g)
            assert (L.ATTN_BWD, bp.variant, bp.hd_image) == bplan
            bargs = (dt, desc, *a, ptr(oo), ptr(dO), ptr(ll), ptr(delta))
            ops.attn_bwd(*bargs, *g)
            dqkv2 = torch.zeros_like(dqkv)
            ops.attn_bwd(*bargs, *_addrs(ptr(dqkv2), off, ko, vo, es))
            h = dqkv.cpu()
            assert torch.equal(dqkv[off:], dqkv2[off:]), f"{mode} backward not deterministic"
            assert off == 0 or bool(h[0] == CANARY), "backward wrote in front of dq"
            for nm, start in (("dq", off), ("dk", off + ko), ("dv", off + vo)):
                ratios[f"{nm}_{mode}"] = _ratio(_view(h, desc, start), ref[nm], bnd[nm])
            # column sums: bitwise the same gradients, rows_out == the plan's rows, partials within a float64 column-sum bound
            cp = ops.attn_plan(L.ATTN_BWD_COLSUM, dt, desc, *a, ptr(dO), *g)
            part = ops.ColsumPartial(B * max(T // 64, 1), 3 * H * hd, torch.device(DEV))
            dqkv3 = torch.zeros_like(dqkv)
            took = ops.attn_bwd_colsum(*bargs, *_addrs(ptr(dqkv3), off, ko, vo, es), part)
            assert took == (cp.colsum_rows > 0) == (bp.variant != L.AV_ROWWISE)
            if took:
                R = part.rows.value
                assert R == cp.colsum_rows and torch.equal(dqkv3[off:], dqkv[off:])
                part2 = ops.ColsumPartial(B * max(T // 64, 1), 3 * H * hd, torch.device(DEV))
                assert ops.attn_bwd_colsum(*bargs, *_addrs(ptr(torch.zeros_like(dqkv)), off, ko, vo, es), part2)
                assert torch.equal(part.buf[:R], part2.buf[:R]), "column-sum partials not deterministic"
                cols = torch.cat([_view(h, desc, st).double().permute(1, 3, 0, 2).reshape(H * hd, -1) for st in (off, off + ko, off + vo)])
                got = part.buf[:R].double().sum(0).cpu()
                assert bool(((got - cols.sum(-1)).abs() <= 2.0 ** -24 * (R + 64) * cols.abs().sum(-1)).all()), "column sums"
    for key, r in ratios.items():
        record_property(f"ratio_{key}", f"{r:.4f}")
    record_property("variants", f"{L.AV_NAMES[fplan[1]]}/{fplan[2]} {L.AV_NAMES[bplan[1]]}/{bplan[2]}")
    assert max(ratios.values()) <= 1.0, f"err / bound over 1: {ratios}"


def test_attention_cases_cover_every_kernel():
    """the (direction, variant, hd_image) set the parity cases run is the whole set the plan can reach"""
    ran = set()
    for name in CASES:
        ran.update(_case_plans(name))
    reachable = ({(L.ATTN_FWD, L.AV_ROWWISE, 0), (L.ATTN_BWD, L.AV_ROWWISE, 0), (L.ATTN_FWD, L.AV_FWD_BIG, 64), (L.ATTN_FWD, L.AV_FWD_BIG, 96)}
                 | {(L.ATTN_FWD, v, i) for v in (L.AV_FWD_T64, L.AV_FWD_G1) for i in (32, 64, 96, 128)}
                 | {(L.ATTN_FWD, L.AV_FWD_G2, i) for i in (32, 64, 96)}
                 | {(L.ATTN_BWD, v, i) for v in (L.AV_BWD_T64, L.AV_BWD_G1) for i in (32, 64, 96, 128)}
                 | {(L.ATTN_BWD, L.AV_BWD_G2, 96)}
                 | {(L.ATTN_BWD, v, i) for v in (L.AV_BWD_BIG_NT2, L.AV_BWD_BIG_NT4) for i in (64, 96)})
    missing = sorted((d, L.AV_NAMES[v], i) for d, v, i in reachable - ran)
    assert ran == reachable, f"kernels no case reaches: {missing}; unexpected: {sorted(ran - reachable)}"


@pytest.mark.parametrize("what", ["T1025", "BH65536", "colsum_short"])
def test_attention_refusals_launch_nothing(what):
    """refused before any launch: every output buffer keeps its canary"""
    B, H, T, hd = {"T1025": (1, 1, 1025, 64), "BH65536": (1, 65536, 64, 8), "colsum_short": (2, 2, 256, 64)}[what]
    D = H * hd
    desc = ops.attn_desc_token_major(B, H, T, hd)
    qkv = torch.zeros(B * T, 3 * D, device=DEV, dtype=torch.bfloat16)
    do = torch.zeros(B * T, D, device=DEV, dtype=torch.bfloat16)
    o = torch.full((B * T, D), CANARY, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B * H * T,), CANARY, device=DEV)
    delta = torch.full((B * H * T,), CANARY, device=DEV)
    dqkv = torch.full_like(qkv, CANARY)
    q, g = ptr(qkv), ptr(dqkv)
    bargs = (BF16, desc, q, q + 2 * D, q + 4 * D, ptr(o), ptr(do), ptr(lse), ptr(delta), g, g + 2 * D, g + 4 * D)
    cap = B * max(T // 64, 1)                 # the capacity vaw_attn_bwd_colsum checks
    big = torch.full((cap + 64, 3 * D), CANARY, device=DEV)
    part = ops.ColsumPartial(1, 3 * D, torch.device(DEV))
    if what == "colsum_short":
        part.buf = big[:cap - 1]
        with pytest.raises(vaw_amd.VawError):
            ops.attn_bwd_colsum(*bargs, part)
    else:
        with pytest.raises(vaw_amd.VawError):
            ops.attn_fwd(BF16, desc, q, q + 2 * D, q + 4 * D, ptr(o), ptr(lse))
        with pytest.raises(vaw_amd.VawError):
            ops.attn_bwd(*bargs)
        part.buf = big[:cap]
        with pytest.raises(vaw_amd.VawError):
            ops.attn_bwd_colsum(*bargs, part)
    torch.cuda.synchronize()
    for t in (o, lse, delta, dqkv, big):
        assert bool((t == CANARY).all())

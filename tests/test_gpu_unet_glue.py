"""Direct float64 parity of the hand-written kernels the whole-model UNet tests only reach in their easiest case: the skinny conv3x3
weight gradient and the narrow-side conv3x3 at ragged chunks / second channel blocks / every small channel count, the
resblock_updown=False and use_scale_shift_norm=False glue (subsample2, rowvec_add, rowvec_sum), the optimizer tail (sumsq, fused
AdamW + EMA in its host- and device-scalar forms, ema, casts) and the second trip of the capped 16-byte data-movement loops.

Every reference is a plain float64 torch statement of the operation on the CPU, from the inputs the kernel is handed (for bf16:
the already-rounded ones).  Where the inputs are small integers the f32 result is exact in any summation order as long as every
partial sum stays below 2^24; the bound is stated next to each case and the comparison is torch.equal.  bf16 outputs of exact
sums are compared bitwise with ref.to(bfloat16): from_f32<bf16_t> (csrc/common.h) is the compiler's float -> __bf16 conversion,
round to nearest even.  Outputs and workspaces are NaN-filled before the call and carry a canary tail that must come back intact.
Run on the MI355X box: pytest -m gpu."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vaw_amd._lib import BF16, F32, lib, ptr, stream_ptr

DEV = "cuda"
NAN = float("nan")
TAIL = 64                 # canary elements behind every output
CANARY = -7.0             # exact in bf16
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -24            # unit roundoff of f32


def _dt(dtype):
    return F32 if dtype == torch.float32 else BF16


def _name(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


def _geo_id(geo):
    return "x".join(str(v) for v in geo)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _ints(g, *shape, lo=-2, hi=2):
    """integers of [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _nhwc(x):   # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _guarded(n, dtype, fill=NAN):
    """n elements of `fill` (a number or a tensor of n values) with TAIL canary elements behind them, on the device"""
    buf = torch.full((n + TAIL,), CANARY, device=DEV, dtype=dtype)
    buf[:n] = fill
    return buf


def _tail_intact(buf, n):
    return buf.numel() == n + TAIL and bool((buf[n:] == CANARY).all())


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------------
# 1. vaw_conv3x3_wgrad_small
# ------------------------------------------------------------------------------------------------
WGRAD_GEOS = [            # (B, H, W, Ci, Co)
    (3, 5, 7, 3, 64),     # M = 105: a single partial chunk, small-in
    (2, 19, 21, 3, 264),  # M = 798: 4 chunks, ragged last, chunks straddle image boundaries, second channel block with 8 live lanes
    (5, 24, 20, 1, 8),    # M = 2400: 10 chunks, the fold loop takes two trips with a remainder; S = 1
    (2, 19, 21, 2, 40),   # S = 2
    (2, 19, 21, 4, 320),  # S = 4
    (3, 5, 7, 64, 3),     # small-out mirrors of the rows above
    (2, 19, 21, 264, 3),
    (5, 24, 20, 8, 1),
    (2, 19, 21, 320, 4),
    (2, 6, 6, 3, 3),      # both sides <= 4: the entry takes the small-in branch
    (2, 6, 6, 4, 2),
]


def _wgrad_ref(x, dy):
    """[B,Ci,H,W], [B,Co,H,W] float64 -> the weight gradient of conv3x3 pad 1 in the kernel's layout [Co][3][3][Ci]"""
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w, padding=1) * dy).sum().backward()
    return w.grad.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _wgrad_int_case(geo):
    """integer inputs and their float64 weight gradient, computed once per geometry and shared by both dtypes (read only)"""
    B, H, W, Ci, Co = geo
    g = _gen(*geo)
    x, dy = _ints(g, B, Ci, H, W), _ints(g, B, Co, H, W)
    return x, dy, _wgrad_ref(x, dy).reshape(-1)


def _wgrad_call(dtype, geo, xd, dyd, dw, beta):
    B, H, W, Ci, Co = geo
    need = lib().vaw_conv3x3_wgrad_small_workspace_floats(B, H, W, Ci, Co)
    assert need == -(-B * H * W // 256) * 9 * Ci * Co
    ws = _guarded(need, torch.float32)
    rc = lib().vaw_conv3x3_wgrad_small(_dt(dtype), ptr(dyd), ptr(xd), ptr(dw), beta, B, H, W, Ci, Co, ptr(ws), need, stream_ptr())
    assert rc == 0, lib().vaw_last_error_string().decode()
    torch.cuda.synchronize()
    assert _tail_intact(ws, need), "the chunk partials ran past the workspace"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", WGRAD_GEOS, ids=_geo_id)
def test_wgrad_small_integer_data_is_exact(dtype, geo):
    """x, dy in [-2, 2]: every product is at most 4 in magnitude and a weight sums at most M <= 2400 of them, so every partial sum
    of the chunk loop, the slab groups and the final fold is an integer of magnitude <= 9600 < 2^24; beta * dw adds at most 6 (an
    integer: beta = 1 onto ones, beta = 0.5 onto even integers).  All exact in f32, in any order."""
    B, H, W, Ci, Co = geo
    x, dy, ref = _wgrad_int_case(geo)
    n = 9 * Ci * Co
    xd, dyd = _nhwc(x).to(dtype).to(DEV), _nhwc(dy).to(dtype).to(DEV)
    even = 2 * _ints(_gen(n, 5), n, lo=-3, hi=3)
    for beta, init in ((0.0, torch.full((n,), NAN, dtype=torch.float64)), (1.0, torch.ones(n, dtype=torch.float64)), (0.5, even)):
        dw = _guarded(n, torch.float32, init.float())
        _wgrad_call(dtype, geo, xd, dyd, dw, beta)
        want = ref if beta == 0.0 else beta * init + ref
        got = dw[:n].cpu().double()
        bad = (got != want).nonzero().flatten()
        assert torch.equal(got, want), (f"beta={beta}: {bad.numel()} of {n} weights differ, first [co,tap,ci]="
                                        f"{np.unravel_index(int(bad[0]), (Co, 9, Ci))} got {got[bad[0]]} want {want[bad[0]]}")
        assert _tail_intact(dw, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", [(2, 19, 21, 3, 264), (2, 19, 21, 264, 3)], ids=_geo_id)
def test_wgrad_small_gaussian_data_within_the_summation_bound(dtype, geo):
    """|got - ref| <= (256 + ceil(nchunk / 8) + 8) * 2^-24 * sum |dy * x| elementwise, the sum over the same taps in float64: the
    worst-case error of the kernel's own summation tree (256 sequential multiply-adds per chunk, then the slab groups of the fold
    with ceil(nchunk / 8) adds, then its 8 adds), each rounding at most 2^-24 relative.  Derived, not measured: no extra margin."""
    B, H, W, Ci, Co = geo
    g = _gen(*geo, 11)
    x, dy = torch.randn(B, Ci, H, W, generator=g).to(dtype), torch.randn(B, Co, H, W, generator=g).to(dtype)
    x64, dy64 = x.double(), dy.double()                      # the rounded inputs
    ref, mag = _wgrad_ref(x64, dy64).reshape(-1), _wgrad_ref(x64.abs(), dy64.abs()).reshape(-1)
    n, nchunk = 9 * Ci * Co, -(-B * H * W // 256)
    assert nchunk == 4
    dw = _guarded(n, torch.float32)
    _wgrad_call(dtype, geo, _nhwc(x).to(DEV), _nhwc(dy).to(DEV), dw, 0.0)
    got = dw[:n].cpu().double()
    bound = (256 + -(-nchunk // 8) + 8) * U * mag
    err = (got - ref).abs()
    print(f"wgrad_small gaussian {_name(dtype)} {geo}: max err / bound = {float((err / bound).max()):.4f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), f"max err / bound = {float((err / bound).max())}"
    assert _tail_intact(dw, n)


# ------------------------------------------------------------------------------------------------
# 2. vaw_conv3x3_narrow at the shapes test_gpu_unet.py does not reach
# ------------------------------------------------------------------------------------------------
NARROW_GEOS = [           # (B, H, W, Cn, Cw)
    (3, 11, 13, 2, 264),  # M = 429: ragged against 256 pixels (modes 0, 1) and 32 (mode 2); Cn = 2; second channel block with one 8-group
    (1, 4, 4, 4, 640),    # mode 2: 92160 B of dynamic LDS, above 64 KiB and inside the 96 KiB the entry asks for
    (1, 4, 4, 3, 688),    # mode 2: 74304 B
]


def _narrow_case(geo, mode, with_bias):
    """(device in [M][Cin], device w, device bias or None, float64 reference [M][Cout]) on integer data.
    Bounds: mode 0  |x| <= 2, |w| <= 1, 9 * Cn <= 36 taps, |bias| <= 2: partial sums <= 74;
            mode 1  |dy| <= 2, |w| <= 1, 36 taps: <= 72;
            mode 2  |x|, |w| <= 1, 9 * Cw <= 6192 taps, |bias| <= 2: <= 6194.  All integers below 2^24: f32 is exact in any order."""
    B, H, W, Cn, Cw = geo
    g = _gen(*geo, mode)
    if mode == 0:
        x, w, b = _ints(g, B, Cn, H, W), _ints(g, Cw, Cn, 3, 3, lo=-1, hi=1), _ints(g, Cw)
        ref = F.conv2d(x, w, b if with_bias else None, padding=1)
        src = x
    elif mode == 2:
        x, w, b = _ints(g, B, Cw, H, W, lo=-1, hi=1), _ints(g, Cn, Cw, 3, 3, lo=-1, hi=1), _ints(g, Cn)
        ref = F.conv2d(x, w, b if with_bias else None, padding=1)
        src = x
    else:                                                    # the input gradient of the narrow-out conv
        dy, w, b = _ints(g, B, Cn, H, W), _ints(g, Cn, Cw, 3, 3, lo=-1, hi=1), None
        assert not with_bias
        xr = torch.zeros(B, Cw, H, W, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xr, w, padding=1) * dy).sum().backward()
        ref, src = xr.grad, dy
    return src, w.permute(0, 2, 3, 1).contiguous(), (b if with_bias else None), _nhwc(ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode,with_bias", [(0, True), (0, False), (1, False), (2, True), (2, False)])
@pytest.mark.parametrize("geo", NARROW_GEOS, ids=_geo_id)
def test_conv3x3_narrow_ragged_blocks_and_large_lds(dtype, geo, mode, with_bias):
    B, H, W, Cn, Cw = geo
    src, w, b, ref = _narrow_case(geo, mode, with_bias)
    M, Cout = B * H * W, (Cn if mode == 2 else Cw)
    ind, wd = _nhwc(src).to(dtype).to(DEV), w.to(dtype).to(DEV)
    bd = b.float().to(DEV) if b is not None else None
    out = _guarded(M * Cout, dtype)
    rc = lib().vaw_conv3x3_narrow(_dt(dtype), mode, ptr(ind), ptr(wd), ptr(bd), ptr(out), B, H, W, Cn, Cw, stream_ptr())
    assert rc == 0, (rc, lib().vaw_last_error_string().decode())
    got = out[:M * Cout].cpu().view(M, Cout)
    if dtype == torch.float32:
        assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {ref.numel()} outputs differ"
    else:                                                    # the exact integer sum, rounded once to nearest even
        want = ref.to(torch.bfloat16)
        assert _same_bits(got, want), f"{int((got.float() != want.float()).sum())} of {ref.numel()} outputs differ"
    assert _tail_intact(out, M * Cout)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_conv3x3_narrow_out_declines_above_96k_of_lds(dtype):
    """4 * 9 * 688 * 4 = 99072 B > 96 KiB: -3 and nothing launched (the caller falls back to the GEMM path)."""
    B, H, W, Cn, Cw = 1, 4, 4, 4, 688
    x = torch.ones(B * H * W, Cw, device=DEV, dtype=dtype)
    w = torch.ones(Cn * 9 * Cw, device=DEV, dtype=dtype)
    out = _guarded(B * H * W * Cn, dtype)
    assert lib().vaw_conv3x3_narrow(_dt(dtype), 2, ptr(x), ptr(w), None, ptr(out), B, H, W, Cn, Cw, stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:B * H * W * Cn]).all()) and _tail_intact(out, B * H * W * Cn)


# ------------------------------------------------------------------------------------------------
# 3. vaw_subsample2, vaw_rowvec_add, vaw_rowvec_sum
# ------------------------------------------------------------------------------------------------
SUB_GEOS = [(3, 5, 7, 4), (2, 6, 4, 36), (1, 8, 8, 192)]     # (B, Ho, Wo, C) of mode 0; mode 1 runs (B, 2 Ho, 2 Wo, C)


def _subsample2(dtype, src, B, Ho, Wo, C, mode):
    out = _guarded(B * Ho * Wo * C, dtype)
    assert lib().vaw_subsample2(_dt(dtype), ptr(src), ptr(out), B, Ho, Wo, C, mode, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _tail_intact(out, B * Ho * Wo * C)
    return out[:B * Ho * Wo * C].view(B, Ho, Wo, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", SUB_GEOS, ids=_geo_id)
def test_subsample2_even_pixels_and_zero_stuffing(dtype, geo):
    B, Ho, Wo, C = geo
    g = _gen(*geo)
    x = torch.randn(B, 2 * Ho, 2 * Wo, C, generator=g).to(dtype)
    got = _subsample2(dtype, x.to(DEV), B, Ho, Wo, C, 0).cpu()
    assert _same_bits(got, x[:, ::2, ::2, :].contiguous())
    # the transpose: out [B, 2 Ho, 2 Wo, C] holds y at the even pixels and zeros elsewhere
    y = torch.randn(B, Ho, Wo, C, generator=g).to(dtype)
    want = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=dtype)
    want[:, ::2, ::2, :] = y
    got = _subsample2(dtype, y.to(DEV), B, 2 * Ho, 2 * Wo, C, 1).cpu()
    assert _same_bits(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", SUB_GEOS, ids=_geo_id)
def test_subsample2_adjoint_identity(dtype, geo):
    """<S x, y> == <x, S^T y> on integers of [-2, 2]: both sides sum at most B * Ho * Wo * C <= 12288 products of magnitude <= 4,
    exact in float64 (and the kernels only move values)."""
    B, Ho, Wo, C = geo
    g = _gen(*geo, 3)
    x, y = _ints(g, B, 2 * Ho, 2 * Wo, C), _ints(g, B, Ho, Wo, C)
    Sx = _subsample2(dtype, x.to(dtype).to(DEV), B, Ho, Wo, C, 0).cpu().double()
    STy = _subsample2(dtype, y.to(dtype).to(DEV), B, 2 * Ho, 2 * Wo, C, 1).cpu().double()
    lhs, rhs = float((Sx * y).sum()), float((x * STy).sum())
    assert lhs == rhs and lhs == float((x[:, ::2, ::2, :] * y).sum())


ROWVEC_GEOS = [(3, 35, 4), (2, 1, 68), (5, 64, 192)]         # (B, HW, C)


def _emb_table(g, B, C):
    """The packed emb_layers output of unet.py:_add_emb: f32 [B][ld] with ld = 3 C + 8 > C, the block's row at a column offset."""
    ld, off = 3 * C + 8, C + 4
    assert ld % 4 == 0 and off % 4 == 0 and off + C <= ld
    return torch.randn(B, ld, generator=g), ld, off


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", ROWVEC_GEOS, ids=_geo_id)
def test_rowvec_add_strided_table_at_a_column_offset(dtype, geo):
    """h[b, p, :] += e[b, off : off + C]: one f32 add, rounded once to the activation dtype."""
    B, HW, C = geo
    g = _gen(*geo)
    h = torch.randn(B, HW, C, generator=g).to(dtype)
    e, ld, off = _emb_table(g, B, C)
    n = B * HW * C
    hd, ed = _guarded(n, dtype, h.reshape(-1).to(DEV)), _guarded(B * ld, torch.float32, e.reshape(-1).to(DEV))
    assert lib().vaw_rowvec_add(_dt(dtype), ptr(hd), ptr(ed) + 4 * off, ld, B, HW, C, stream_ptr()) == 0
    want = (h.float() + e[:, None, off:off + C]).to(dtype)
    assert _same_bits(hd[:n].cpu().view(B, HW, C), want)
    assert _tail_intact(hd, n)
    assert _same_bits(ed[:B * ld].cpu().view(B, ld), e) and _tail_intact(ed, B * ld)        # the table is only read


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geo", ROWVEC_GEOS + [(2, 3, 68), (3, 3, 4)], ids=_geo_id)       # HW = 3: fewer rows than the 4 row groups
def test_rowvec_sum_integer_data_is_exact(dtype, geo):
    """de[b, off : off + C] = beta * de + sum_p dh[b, p, :] on integers of [-2, 2]: a column sums at most HW <= 64 of them, every
    partial sum (4 row groups, then their fold, then beta * de <= 6) is an integer of magnitude <= 134 < 2^24: exact in f32."""
    B, HW, C = geo
    g = _gen(*geo, 1)
    dh = _ints(g, B, HW, C)
    ref = dh.sum(1)                                                                         # float64 [B, C]
    ld, off = 3 * C + 8, C + 4                                                              # the strided table of rowvec_add
    even = 2 * _ints(g, B, C, lo=-3, hi=3)
    dhd = dh.to(dtype).reshape(-1).to(DEV)
    for beta, init in ((0.0, torch.full((B, C), NAN, dtype=torch.float64)), (1.0, torch.ones(B, C, dtype=torch.float64)), (0.5, even)):
        de = torch.full((B, ld), CANARY)
        de[:, off:off + C] = init.float()
        ded = _guarded(B * ld, torch.float32, de.reshape(-1).to(DEV))
        assert lib().vaw_rowvec_sum(_dt(dtype), ptr(dhd), ptr(ded) + 4 * off, ld, B, HW, C, beta, stream_ptr()) == 0
        got = ded[:B * ld].cpu().view(B, ld)
        want = ref if beta == 0.0 else beta * init + ref
        assert torch.equal(got[:, off:off + C].double(), want), f"beta={beta}"
        outside = torch.ones(B, ld, dtype=torch.bool)
        outside[:, off:off + C] = False
        assert bool((got[outside] == CANARY).all()) and _tail_intact(ded, B * ld), f"beta={beta}: a float outside the windows changed"


# ------------------------------------------------------------------------------------------------
# 4. optimizer tail
# ------------------------------------------------------------------------------------------------
HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, decay=0.999)
ADAM_N = [3, 4096 * 2, 4096 * 2 + 4 * 37 + 3, 4096 * 2050 + 5]      # the last is above the 2048-tile grid cap
ADAM_SWITCH_N = 4096 * 2 + 4 * 37 + 3                                # two whole tiles, 37 float4 of a partial tile, 3 elements


def _f32(v):
    """the value a float argument has once it is a C float: what the kernel computes from"""
    return float(np.float32(v))


def _sumsq(gbuf, n, out, accumulate):
    need = lib().vaw_sumsq_workspace_floats()
    ws = _guarded(need, torch.float32)
    assert lib().vaw_sumsq(ptr(gbuf), n, ptr(out), accumulate, ptr(ws), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _tail_intact(ws, need)


def _adam_ref_step(st, g, step, ss, clip, has_ema):
    """float64 restatement of adam_one (csrc/elementwise.hip) on the f32 scalars the kernel is handed: decoupled decay, the m and v
    updates, bias correction, the update, then EMA; the gradient scaled by the clip factor min(1, clip / (sqrt(sumsq) + 1e-6))."""
    lr, b1, b2, eps, wd, d = (_f32(HP[k]) for k in ("lr", "b1", "b2", "eps", "wd", "decay"))
    bc1, bc2 = _f32(1.0 - HP["b1"] ** step), _f32(1.0 - HP["b2"] ** step)
    gs = min(1.0, _f32(clip) / (math.sqrt(ss) + _f32(1e-6))) if clip > 0 else 1.0
    gg = g * gs
    p = st["p"] * (1.0 - lr * wd)
    m = st["m"] + (gg - st["m"]) * (1.0 - b1)
    v = st["v"] * b2 + (1.0 - b2) * gg * gg
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    st.update(p=p, m=m, v=v)
    if has_ema:
        st["e"] = st["e"] * d + p * (1.0 - d)


def _adam_start(n):
    g0 = _gen(n, 17)
    p0 = torch.randn(n, generator=g0)
    return p0, p0 + 0.01 * torch.randn(n, generator=g0), g0


def _adam_run(path, n, steps=3, ema=True, shadow=True, clip=1.0, zero_grad=1, with_ref=True):
    """`steps` optimizer steps from a fixed start (m = v = 0, as a trainer starts) through vaw_adamw_ema_step (path "host") or
    vaw_adamw_ema_step_dev with hyper = [lr, bc1, bc2] on the device (path "dev"); returns the device buffers (canary tails
    included), the float64 state, and the last gradient as it went in."""
    p0, e0, g0 = _adam_start(n)
    z = torch.zeros(n)
    dev = {k: _guarded(n, torch.float32, t.to(DEV)) for k, t in (("p", p0), ("m", z), ("v", z), ("e", e0))}
    dev["s"] = _guarded(n, torch.bfloat16)
    ref = dict(p=p0.double(), m=z.double(), v=z.double(), e=e0.double())
    ss = torch.full((1,), NAN, device=DEV)
    L = lib()
    for step in range(1, steps + 1):
        # 0.1-sigma gradients; step 2 is 30 times larger, so that even n = 3 has one step with the clip active and one without
        g = torch.randn(n, generator=g0) * (3.0 if step == 2 else 0.1)
        dev["g"] = _guarded(n, torch.float32, g.to(DEV))
        ssv = 0.0
        if clip > 0:
            _sumsq(dev["g"], n, ss, 0)
            ssv = float(ss.cpu().double())
        pe, ps, pss = (ptr(dev["e"]) if ema else None), (ptr(dev["s"]) if shadow else None), (ptr(ss) if clip > 0 else None)
        bc1, bc2 = 1.0 - HP["b1"] ** step, 1.0 - HP["b2"] ** step
        if path == "host":
            rc = L.vaw_adamw_ema_step(ptr(dev["p"]), ptr(dev["g"]), ptr(dev["m"]), ptr(dev["v"]), pe, ps, n, HP["lr"], HP["b1"], HP["b2"],
                                      HP["eps"], HP["wd"], bc1, bc2, HP["decay"], pss, clip, zero_grad, stream_ptr())
        else:
            hyper = torch.tensor([HP["lr"], bc1, bc2], dtype=torch.float32, device=DEV)
            rc = L.vaw_adamw_ema_step_dev(ptr(dev["p"]), ptr(dev["g"]), ptr(dev["m"]), ptr(dev["v"]), pe, ps, n, ptr(hyper), HP["b1"],
                                          HP["b2"], HP["eps"], HP["wd"], HP["decay"], pss, clip, zero_grad, stream_ptr())
        assert rc == 0, L.vaw_last_error_string().decode()
        torch.cuda.synchronize()
        if with_ref:
            _adam_ref_step(ref, g.double(), step, ssv, clip, ema)
    for k, buf in dev.items():
        assert _tail_intact(buf, n), f"{k}: canary tail overwritten"
    return dev, ref, g


def _adam_check(dev, ref, g_in, n, ema, shadow, zero_grad):
    """the tolerances of test_fused_adamw_ema_matches_torch_adamw, after 3 steps from the same start"""
    p = dev["p"][:n].cpu()
    torch.testing.assert_close(p.double(), ref["p"], rtol=1e-5, atol=1e-7)
    if ema:
        torch.testing.assert_close(dev["e"][:n].cpu().double(), ref["e"], rtol=1e-6, atol=1e-7)
    else:
        assert _same_bits(dev["e"][:n].cpu(), _adam_start(n)[1]), "ema = NULL: the buffer was not handed over and must not change"
    if shadow:
        assert _same_bits(dev["s"][:n].cpu(), p.bfloat16())
    else:
        assert bool(torch.isnan(dev["s"][:n]).all())
    if zero_grad:
        assert not bool(dev["g"][:n].view(torch.int32).any()), "zero_grad left a nonzero word (the n % 4 tail included)"
    else:
        assert _same_bits(dev["g"][:n].cpu(), g_in)


@pytest.mark.parametrize("n", ADAM_N)
def test_adamw_dev_scalars_match_host_scalars_bitwise(n):
    """The variant every captured step uses reads lr, bc1, bc2 from device memory and takes sqrt(bc2) itself: the same f32 values,
    so p, m, v, ema, shadow and g come back bit for bit those of the host-scalar entry, which is held to the float64 restatement."""
    host, ref, g_in = _adam_run("host", n)
    _adam_check(host, ref, g_in, n, True, True, 1)
    devp, _, _ = _adam_run("dev", n, with_ref=False)
    for k in ("p", "m", "v", "e", "s", "g"):
        assert _same_bits(host[k], devp[k]), f"{k}: {int((host[k].float() != devp[k].float()).sum())} of {n} elements differ"
    del host, devp, ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("switch", ["no_ema", "no_shadow", "no_clip", "keep_grad", "zero_grad"])
def test_adamw_each_switch_alone(path, switch):
    n = ADAM_SWITCH_N
    ema, shadow = switch != "no_ema", switch != "no_shadow"
    clip, zero_grad = (0.0 if switch == "no_clip" else 1.0), (0 if switch == "keep_grad" else 1)
    dev, ref, g_in = _adam_run(path, n, ema=ema, shadow=shadow, clip=clip, zero_grad=zero_grad)
    _adam_check(dev, ref, g_in, n, ema, shadow, zero_grad)


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 4096 * 2050 + 5])
def test_sumsq_against_float64(n):
    """rtol = 1e-5 of test_fused_adamw_ema_matches_torch_adamw; accumulate = 0 must not read the NaN in the destination."""
    g = torch.randn(n, generator=_gen(n, 23))
    want = float((g.double() ** 2).sum())
    gd = _guarded(n, torch.float32, g.to(DEV))
    out = _guarded(1, torch.float32)
    _sumsq(gd, n, out, 0)
    torch.testing.assert_close(float(out[0]), want, rtol=1e-5, atol=0)
    first = float(out[0].cpu().double())
    _sumsq(gd, n, out, 1)
    torch.testing.assert_close(float(out[0]), first + want, rtol=1e-5, atol=0)
    out[0] = 2.5
    _sumsq(gd, n, out, 1)
    torch.testing.assert_close(float(out[0]), 2.5 + want, rtol=1e-5, atol=0)
    assert _tail_intact(out, 1) and _tail_intact(gd, n)


@pytest.mark.parametrize("n", [1, 1027, 2048 * 256 + 77])             # the last: a second trip of the capped grid
def test_ema_update_against_float64(n):
    """ema = ema * d + src * (1 - d) in f32: 1 - d is exact (d in [0.5, 1]), the two products and the sum round once each, so
    |got - ref| <= (2u + u^2) (|ema * d| + |src * (1 - d)|) with u = 2^-24; 2u + u^2 < 2.000001 u."""
    g = _gen(n, 29)
    e, s = torch.randn(n, generator=g), torch.randn(n, generator=g)
    d = _f32(0.999)
    ed, sd = _guarded(n, torch.float32, e.to(DEV)), _guarded(n, torch.float32, s.to(DEV))
    assert lib().vaw_ema_update(ptr(ed), ptr(sd), n, 0.999, stream_ptr()) == 0
    a, b = e.double() * d, s.double() * (1.0 - d)
    err = (ed[:n].cpu().double() - (a + b)).abs()
    assert bool((err <= 2.000001 * U * (a.abs() + b.abs())).all()), float((err / (U * (a.abs() + b.abs()))).max())
    assert _same_bits(sd[:n].cpu(), s) and _tail_intact(ed, n) and _tail_intact(sd, n)


def _cast_specials():
    t, i = torch.tensor, np.float32
    nxt = lambda v, to: float(np.nextafter(i(v), i(to)))
    return t([1.0 + 2.0 ** -8,                 # exact tie, even neighbour below
              NAN,
              1e-40,                           # f32 denormal (bf16 keeps denormals: 2^-133 steps)
              1.0 + 3 * 2.0 ** -8,             # exact tie, even neighbour above
              -0.0, 0.0, float("inf"), -float("inf"),
              -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),
              nxt(1.0 + 2.0 ** -7, 0.0),       # just under a bf16 step: rounds up to it
              nxt(1.0 + 2.0 ** -8, 0.0),       # just under a tie: rounds down
              nxt(1.0 + 2.0 ** -8, 2.0),       # just over a tie: rounds up
              -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -134, 3 * 2.0 ** -134,            # denormal ties and the smallest denormal
              2.0 ** -126, 3.3895313892515355e38,                                            # smallest normal, the largest bf16
              3.4028234663852886e38,                                                         # the largest f32: rounds to inf
              257.0, 259.0, 1.0 / 3.0, -2.0 / 3.0, 65535.0, 1e-30, -1e30], dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 3, 8, 1027])
def test_cast_bf16_rounds_to_nearest_even_bitwise(n):
    """n = 1, 3: the scalar tail alone; n = 8: the 4-wide body alone; n = 1027: both, every special value in both."""
    sp = _cast_specials()
    src = sp[torch.arange(n) % sp.numel()].clone()
    sd, dd = _guarded(n, torch.float32, src.to(DEV)), _guarded(n, torch.bfloat16)
    assert lib().vaw_cast_bf16(ptr(sd), ptr(dd), n, stream_ptr()) == 0
    got, want = dd[:n].cpu(), src.bfloat16()
    isn = torch.isnan(want)
    assert torch.equal(torch.isnan(got), isn), "NaN must stay NaN and nothing else may become one"
    bg, bw = got.view(torch.int16)[~isn], want.view(torch.int16)[~isn]
    bad = (bg != bw).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} differ, first: src {float(src[~isn][bad[0]])!r} got {float(got[~isn][bad[0]])!r} want {float(want[~isn][bad[0]])!r}"
    assert _tail_intact(dd, n) and _tail_intact(sd, n)


@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0])
@pytest.mark.parametrize("n", [1, 7, 8, 1027])
def test_uncast_bf16_times_scale_bitwise(n, scale):
    """dst = float(src) * scale, one f32 product: bitwise the same product on the CPU."""
    g = _gen(n, 31)
    src = (torch.randn(n, generator=g) * 4.0).bfloat16()
    sp = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 3.3895313892515355e38, 2.0 ** -126, 255.0, -1.0 / 3.0]).bfloat16()
    k = min(n, sp.numel())
    src[n - k:] = sp[:k]                                     # specials at the end: in the scalar tail for n = 7, 1027
    sd, dd = _guarded(n, torch.bfloat16, src.to(DEV)), _guarded(n, torch.float32)
    assert lib().vaw_uncast_bf16(ptr(sd), ptr(dd), n, scale, stream_ptr()) == 0
    want = src.float() * torch.tensor(np.float32(scale))     # f32 times f32, rounded once
    assert want.dtype == torch.float32 and _same_bits(dd[:n].cpu(), want)
    assert _tail_intact(dd, n) and _tail_intact(sd, n)


# ------------------------------------------------------------------------------------------------
# 5. second trip of the capped 16-byte loops (the only large allocations of this file: ~135 MB a tensor)
# ------------------------------------------------------------------------------------------------
BIG_N8 = 8192 * 1024 + 1000       # octets: one trip of the 8192-workgroup grid covers 8192 * 1024 of them, the second is ragged


def test_add_inplace_second_trip_of_the_capped_grid():
    n = 8 * BIG_N8
    g = torch.Generator(device=DEV).manual_seed(41)
    d0 = torch.randn(n, device=DEV, generator=g).bfloat16()
    sr = torch.randn(n, device=DEV, generator=g).bfloat16()
    d = torch.cat([d0, torch.full((TAIL,), CANARY, device=DEV, dtype=torch.bfloat16)])
    assert lib().vaw_add_inplace(BF16, ptr(d), ptr(sr), n, stream_ptr()) == 0
    want = torch.add(d0, sr)                                 # f32 sum of two bf16 values rounded once: what the kernel does
    ok, tail = _same_bits(d[:n], want), _tail_intact(d, n)
    del d0, sr, d, want
    torch.cuda.empty_cache()
    assert ok and tail


def test_concat_channels_second_trip_of_the_capped_grid():
    Ca, Cb = 24, 40
    M = BIG_N8 // ((Ca + Cb) // 8)
    assert M * (Ca + Cb) == 8 * BIG_N8
    g = torch.Generator(device=DEV).manual_seed(43)
    a = torch.randn(M, Ca, device=DEV, generator=g).bfloat16()
    b = torch.randn(M, Cb, device=DEV, generator=g).bfloat16()
    cat = _guarded(M * (Ca + Cb), torch.bfloat16)
    assert lib().vaw_concat_channels(BF16, ptr(a), ptr(b), ptr(cat), M, Ca, Cb, 0, stream_ptr()) == 0
    want = torch.cat([a, b], 1)
    ok_cat = _same_bits(cat[:M * (Ca + Cb)].view(M, Ca + Cb), want) and _tail_intact(cat, M * (Ca + Cb))
    del cat
    a2, b2 = _guarded(M * Ca, torch.bfloat16), _guarded(M * Cb, torch.bfloat16)
    assert lib().vaw_concat_channels(BF16, ptr(a2), ptr(b2), ptr(want), M, Ca, Cb, 1, stream_ptr()) == 0
    ok_split = (_same_bits(a2[:M * Ca].view(M, Ca), a) and _same_bits(b2[:M * Cb].view(M, Cb), b) and
                _tail_intact(a2, M * Ca) and _tail_intact(b2, M * Cb))
    del a, b, a2, b2, want
    torch.cuda.empty_cache()
    assert ok_cat and ok_split

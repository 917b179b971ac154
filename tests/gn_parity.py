"""Float64 reference, bounds, case table and simulated kernels for GroupNorm (csrc/groupnorm.hip: vaw_groupnorm_fwd / _apply / _bwd),
imported by test_gn_parity_cpu.py and test_gpu_groupnorm.py; no GPU needed, tensors live wherever the caller puts them.

Reference.  From the stored values of the bf16 / f32 inputs, in float64: per (sample, group) mean and rstd = 1 / sqrt(var + eps) (biased
variance), y = act(((x - mean) rstd gamma + beta) [(1 + scale) + shift]), and by autograd for a given dout: dx (+ dx_add), dgamma, dbeta,
dscale, dshift; dgamma and dbeta are grad_beta times what the buffers held plus the gradient (what they held is not read at grad_beta 0).

Bounds.  Outputs follow the rule of test_gpu_rows.py: f32  |err| <= 1e-5 |ref| + 1e-5 rms, with rms(ref) for the per-element outputs y and
dx and sqrt(terms) rms(summands) for the reduced outputs dgamma, dbeta (B HW summands), dscale, dshift (HW summands); bf16 outputs within
one bf16 ulp of the float64 value plus the same floor.  The statistics are bounded from the launch: with n the longest chain of f32
additions a chunk partial goes through (quad: ceil(min(rows, HW) / 16) + 16, flat: ceil(min(rows, HW) / rpi) + rpi; chunks and channels
are folded in double) and u = 2^-24,
    |d mean| <= n u mean|x| + u |mean|            (n roundings of partial sums that never exceed sum |x|, one conversion to f32)
    |d rstd| / rstd <= 1.5 n u mean(x^2) / (var + eps) + 2 u
(the sums of x and x^2 err by n u mean|x| and (n + 1) u mean(x^2) per element; var = E[x^2] - m^2 takes the second and 2 |m| times the
first, together at most 3 n u mean(x^2); rstd moves by half of that over var + eps; two conversions).  This charges the cancellation of
E[x^2] - m^2 to the data's own conditioning.
PROPAGATED names the outputs whose bound also carries those statistics bounds pushed through the passes (stat_term()).

Regimes.  normal: x = 1.5 N(0, 1) + 0.3, Gaussian gamma, beta, FiLM rows and dout, eps = 1e-5.  offset: the same with the mean at eight
standard deviations (+ 12).  exact: x = m_g +- 2^k_g per (sample, group), m_g in -3 .. 3, k_g in {0, 1, 2}, the signs of a group summing
to zero, small integers everywhere else, eps = 0, no SiLU: mean = m_g and rstd = 2^-k_g, and with cg HW a power of two every quantity
either mapping forms (P, Q, S1 / N, K2, K3, dx) is exact in f32, so f32 outputs must equal the reference and bf16 outputs the reference
rounded to bf16 -- a wrong group, lane, chunk or row is an inequality.  Where cg HW is even but no power of two only the forward is exact
and the backward is held to the bounds.

simulate() restates the passes in torch f32 on the lanes and chunks of the planned launch, rounding where the kernels round, with one
injected fault of FAULTS: the comparator's own test object.

MEASURED_GN: worst err / bound per (mapping, pass, regime) on the MI355X (pytest -m gpu tests/test_gpu_groupnorm.py -s)."""
import math
import zlib

import torch

U = 2.0 ** -24
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
TARGET_FIELDS = ("variant", "rows", "nch", "nt", "rpi", "last", "bg128", "bg256")
OUTPUTS = ("mean", "rstd", "y", "dx", "dgamma", "dbeta", "dscale", "dshift")
PASS_OF = {"mean": "stats", "rstd": "stats", "y": "fwd", "dx": "bwd_dx", "dgamma": "bwd_sums", "dbeta": "bwd_sums", "dscale": "bwd_sums",
           "dshift": "bwd_sums"}
# Outputs whose bound carries stat_term().  Every pass is computed from the f32 mean and rstd, so what the statistics bounds allow
# reaches every output.  Against the bare output rule the unchanged kernels missed 11 of the 108 cases on the MI355X (worst err / bound
# in brackets), all of them groups whose own conditioning is poor, and the f32 restatement of the passes (simulate(), no fault) misses
# the same ones on the CPU:
#   cg HW = 1 (quad_bf16_33x1x4_g4_offset [y 10], quad_bf16_17x1x12_g12_normal [y 2.1], quad_bf16_1x1x36_g36_offset [y 50]): var = 0,
#       rstd = eps^-1/2 = 316; y = x a1 + b1 cancels x rstd gamma against mean rstd gamma, two terms of 316 |x| whose roundings
#       (u |mean| rstd |gamma|: dy/dmean times the mean's own conversion to f32) stand against a reference of beta alone
#   cg HW = 3 at the offset mean (quad_f32_17x3x36_g36_offset [dx 201, y 123, dscale 46, dgamma 39, dshift 11, dbeta 3.0],
#       quad_f32_17x1x36_g12_offset [dx 25, dscale 7.2, y 5.1]): a handful of values at 12 +- 1.5, mean(x^2) / var of several hundred
#   the offset mean in f32 and one flat bf16 case (quad_f32_17x513x12_g12_offset [dx 3.8, y 1.5, dscale 1.01], ..17x513x68_g17.. [dx 2.2],
#       ..17x16x12_g4.. [dx 1.5], ..17x1040x4_g1.. [dx 1.2], quad_f32_33x3x12_g12_normal [dx 1.1], flat_256x1024x8_g2_offset [dx 2.0]):
#       mean(x^2) / var = 65, the statistics bound allows rstd 3e-4 relative at n = 48 and a few 1e-5 of it arrive; the flat dx =
#       P d - K3 x - K2 cancels K3 x against K3 mean in K2, again dx/dmean times u |mean|
# No other miss was seen.  In the normal regime the term is n u (about 3e-6 relative at n = 48) beside the rule's 1e-5; in the exact
# regime nothing is bounded, so it cannot hide a wrong lane, group, chunk or row there.
PROPAGATED = ("y", "dx", "dgamma", "dbeta", "dscale", "dshift")

# Worst err / bound on the MI355X over the 108 cases, bounds as they stand (with the propagated term): (mapping and dtype, pass, regime)
# -> ratio; passes: stats = mean, rstd; fwd = y; bwd_dx = dx; bwd_sums = dgamma, dbeta, dscale, dshift.  The bf16 y and dx sit at 0.5:
# the storage term is one ulp and correct rounding errs by half of one, so these kernels round the f32 value they should.  Everything
# stored in f32 stays below 0.12: the bounds are worst cases in n, the sums err like a random walk.  exact: 0 is "every element equal to
# the reference"; all 37 exact cases came back so in mean, rstd and y, and the 11 whose cg HW is a power of two in every output.  The
# non-zero bwd figures of that regime are the other 26, whose backward is held to the bounds.
MEASURED_GN = {
    ("quad_f32", "stats", "normal"): 0.096, ("quad_f32", "stats", "offset"): 0.110, ("quad_f32", "stats", "exact"): 0.0,
    ("quad_f32", "fwd", "normal"): 0.031, ("quad_f32", "fwd", "offset"): 0.076, ("quad_f32", "fwd", "exact"): 0.0,
    ("quad_f32", "bwd_dx", "normal"): 0.111, ("quad_f32", "bwd_dx", "offset"): 0.070, ("quad_f32", "bwd_dx", "exact"): 0.012,
    ("quad_f32", "bwd_sums", "normal"): 0.031, ("quad_f32", "bwd_sums", "offset"): 0.058, ("quad_f32", "bwd_sums", "exact"): 0.0,
    ("quad_bf16", "stats", "normal"): 0.046, ("quad_bf16", "stats", "offset"): 0.037, ("quad_bf16", "stats", "exact"): 0.0,
    ("quad_bf16", "fwd", "normal"): 0.499, ("quad_bf16", "fwd", "offset"): 0.498, ("quad_bf16", "fwd", "exact"): 0.0,
    ("quad_bf16", "bwd_dx", "normal"): 0.500, ("quad_bf16", "bwd_dx", "offset"): 0.499, ("quad_bf16", "bwd_dx", "exact"): 0.496,
    ("quad_bf16", "bwd_sums", "normal"): 0.038, ("quad_bf16", "bwd_sums", "offset"): 0.031, ("quad_bf16", "bwd_sums", "exact"): 0.0,
    ("flat_bf16", "stats", "normal"): 0.043, ("flat_bf16", "stats", "offset"): 0.026, ("flat_bf16", "stats", "exact"): 0.0,
    ("flat_bf16", "fwd", "normal"): 0.500, ("flat_bf16", "fwd", "offset"): 0.498, ("flat_bf16", "fwd", "exact"): 0.0,
    ("flat_bf16", "bwd_dx", "normal"): 0.500, ("flat_bf16", "bwd_dx", "offset"): 0.499, ("flat_bf16", "bwd_dx", "exact"): 0.500,
    ("flat_bf16", "bwd_sums", "normal"): 0.084, ("flat_bf16", "bwd_sums", "offset"): 0.016, ("flat_bf16", "bwd_sums", "exact"): 0.0,
}


def rnd(t, dt):
    return t.to(TORCH_DT[dt]).double()


# ------------------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------------------
def _quad_target(B, HW, G):
    nch = -(-HW // 512)
    return ("quad", 512, nch, 0, 0, HW - (nch - 1) * 512, B * G > 128, B * G > 256)


def _rot(i):
    """(film, silu, add, grad_beta) of the i-th case: periods 3, 2, 2 (shifted) and 3 (on i // 2), so that they mix"""
    return (None, "3C", "2C8")[i % 3], i % 2 == 0, (i // 2) % 2 == 0, (0.0, 1.0, 0.5)[(i // 2) % 3]


def exact_fwd_possible(c):
    return (c["C"] // c["G"] * c["HW"]) % 2 == 0


def exact_bwd(c):
    n = c["C"] // c["G"] * c["HW"]
    return c["regime"] == "exact" and n & (n - 1) == 0


def _build_cases():
    out = {}

    def add(name, dt, switch, shape, G, regime, target, i):
        assert name not in out, name
        B, HW, C = shape
        film, silu, addx, gbeta = _rot(i)
        c = dict(name=name, dt=dt, switch=switch, B=B, HW=HW, C=C, G=G, regime=regime, film=film, silu=silu and regime != "exact",
                 add=addx, grad_beta=gbeta, eps=0.0 if regime == "exact" else 1e-5, target=dict(zip(TARGET_FIELDS, target)))
        assert regime != "exact" or exact_fwd_possible(c), name
        out[name] = c

    # ---- flat by shape (switch -1): (B, HW, C), G, (rows, nch, nt, rpi, last chunk); each once in the normal regime and once in
    # the exact one (or the offset one where cg HW is odd)
    by_shape = [((512, 16, 8), 8, (512, 1, 256, 256, 16)), ((256, 513, 8), 2, (512, 2, 256, 256, 1)),
                ((256, 1024, 8), 2, (512, 2, 256, 256, 512)), ((256, 257, 16), 4, (256, 2, 256, 128, 1)),
                ((256, 512, 16), 4, (256, 2, 256, 128, 256)), ((128, 385, 24), 3, (128, 4, 255, 85, 1))]
    # ---- flat forced (switch 1)
    forced = [((2, 130, 2048), 32, (128, 2, 256, 1, 2)), ((2, 40, 1032), 24, (128, 1, 129, 1, 40)), ((3, 129, 136), 1, (128, 2, 255, 15, 1)),
              ((3, 129, 136), 17, (128, 2, 255, 15, 1)), ((5, 64, 64), 64, (128, 1, 256, 32, 64)), ((2, 130, 96), 32, (128, 2, 252, 21, 2)),
              ((2, 33, 192), 32, (128, 1, 240, 10, 33)), ((3, 64, 40), 10, (128, 1, 255, 51, 64)), ((2, 40, 1032), 43, (128, 1, 129, 1, 40))]
    i = 0
    for switch, table in ((-1, by_shape), (1, forced)):
        for shape, G, (rows, nch, nt, rpi, last) in table:
            B, HW, C = shape
            tgt = ("flat", rows, nch, nt, rpi, last, B * G > 128, B * G > 256)
            probe = dict(C=C, G=G, HW=HW)
            for regime in ("normal", "exact" if exact_fwd_possible(probe) else "offset"):
                add("flat{}_{}x{}x{}_g{}_{}".format("" if switch < 0 else "f", *shape, G, regime), "bf16", switch, shape, G, regime, tgt, i)
                i += 1
    add("flatf_3x129x136_g17_offset", "bf16", 1, (3, 129, 136), 17, "offset", ("flat", 128, 2, 255, 15, 1, False, False), i)
    add("flat_256x512x16_g4_offset", "bf16", -1, (256, 512, 16), 4, "offset", ("flat", 256, 2, 256, 128, 256, True, True), i + 1)
    add("flat_256x1024x8_g2_offset", "bf16", -1, (256, 1024, 8), 2, "offset", ("flat", 512, 2, 256, 256, 512, True, True), i + 3)

    # ---- quad: every (C, G) meets every HW; B, the dtype, the switch and the regime rotate (five consecutive cases of a (C, G) pair
    # see every B and both dtypes).  C % 8 == 4 keeps bf16 on the quad kernels under any switch.
    pairs = [(C, G) for C in (4, 12, 36, 68, 100) for G in sorted({1, C // 4, C // 3 if C % 3 == 0 else 1, C}) if G <= 64 and C % G == 0]
    i = 0
    for C, G in pairs:
        for HW in (1, 3, 16, 513, 1040):
            B = (1, 17, 33)[i % 3]
            while B * HW * C > 2_000_000:
                B = {33: 17, 17: 1}[B]
            dt = ("f32", "bf16")[i % 2]
            probe = dict(C=C, G=G, HW=HW)
            regime = ("normal", "exact", "offset")[(i // 2) % 3]
            if regime == "exact" and not exact_fwd_possible(probe):
                regime = ("normal", "offset")[(i // 3) % 2]
            add(f"quad_{dt}_{B}x{HW}x{C}_g{G}_{regime}", dt, (-1, 1, 0)[i % 3], (B, HW, C), G, regime, _quad_target(B, HW, G), i)
            i += 1
    add("quad_bf16_1x4x2056_g8_normal", "bf16", 1, (1, 4, 2056), 8, "normal", _quad_target(1, 4, 8), 3)
    add("quad_bf16_1x4x2056_g8_exact", "bf16", -1, (1, 4, 2056), 8, "exact", _quad_target(1, 4, 8), 4)
    add("quad_bf16_2x64x64_g32_byshape_normal", "bf16", -1, (2, 64, 64), 32, "normal", _quad_target(2, 64, 32), 0)
    add("quad_bf16_2x64x64_g32_byshape_exact", "bf16", -1, (2, 64, 64), 32, "exact", _quad_target(2, 64, 32), 1)
    add("quad_f32_2x64x2048_g32_exact", "f32", 1, (2, 64, 2048), 32, "exact", _quad_target(2, 64, 32), 2)
    return out


CASES = _build_cases()


def film_layout(c):
    """(film_ld, scale column, shift column, dfilm_ld, dscale column, dshift column): the engine's 3 C rows, or rows of 2 C + 8 with a
    column offset of 4; the gradient rows take the other layout, so dfilm_ld != film_ld"""
    C = c["C"]
    a, b = (3 * C, C, 2 * C), (2 * C + 8, 4, 4 + C)
    return (a + b) if c["film"] == "3C" else (b + a)


def chain(c):
    t = c["target"]
    r = min(t["rows"], c["HW"])
    lanes = t["rpi"] if t["variant"] == "flat" else 16
    return -(-r // lanes) + lanes


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """name -> float64 CPU tensor holding values of the operand's storage format: x, dout, dx_add [B][HW][C] (the activation dtype),
    gamma, beta [C], emb [B][film_ld] (f32; scale and shift are column blocks of it), dgamma_old, dbeta_old [C] (NaN at grad_beta 0)"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    B, HW, C, G, dt = c["B"], c["HW"], c["C"], c["G"], c["dt"]
    cg = C // G
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    t = {}
    if c["regime"] == "exact":
        n = cg * HW
        m, k = ri(-3, 3, B, G, 1), ri(0, 2, B, G, 1)
        order = torch.rand(B, G, n, generator=g).argsort(2)
        sign = torch.where(order < n // 2, 1.0, -1.0).double()
        xg = m + sign * torch.pow(2.0, k)                                   # [B][G][HW cg]
        t["x"] = xg.view(B, G, HW, cg).permute(0, 2, 1, 3).reshape(B, HW, C).contiguous()
        t["dout"] = ri(-2, 2, B, HW, C)
        if c["add"]:
            t["dx_add"] = ri(-2, 2, B, HW, C)
        gam = ri(1, 2, C) * torch.where(ri(0, 1, C) > 0, 1.0, -1.0).double()
        t["gamma"], t["beta"] = gam, ri(-2, 2, C)
        if c["film"]:
            t["emb"] = ri(-2, 1, B, film_layout(c)[0])
        old = lambda: ri(-4, 4, C)
    else:
        off = 12.0 if c["regime"] == "offset" else 0.3
        t["x"] = rnd(1.5 * r(B, HW, C) + off, dt)
        t["dout"] = rnd(r(B, HW, C), dt)
        if c["add"]:
            t["dx_add"] = rnd(r(B, HW, C), dt)
        t["gamma"], t["beta"] = rnd(0.5 * r(C) + 1.0, "f32"), rnd(0.2 * r(C), "f32")
        if c["film"]:
            t["emb"] = rnd(0.3 * r(B, film_layout(c)[0]), "f32")
        old = lambda: rnd(r(C), "f32")
    for k in ("dgamma_old", "dbeta_old"):
        t[k] = old() if c["grad_beta"] != 0.0 else torch.full((C,), float("nan"), dtype=torch.float64)
    return t


def _film(c, t):
    if not c["film"]:
        return None, None
    _, so, ho = film_layout(c)[:3]
    C = c["C"]
    return t["emb"][:, so:so + C], t["emb"][:, ho:ho + C]


def _per_channel(v, cg):
    """[B][G] -> [B][1][C]"""
    return v.repeat_interleave(cg, dim=1)[:, None, :]


def _old(c, t, k):
    return c["grad_beta"] * t[k] if c["grad_beta"] != 0.0 else torch.zeros_like(t[k])


# ------------------------------------------------------------------------------------------------------------------------------
# reference and bounds
# ------------------------------------------------------------------------------------------------------------------------------
def reference(c, t):
    """name -> float64 reference of every output, and `aux`: what the bounds need (summands of the reduced outputs, group moments)"""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg = C // G
    x = t["x"].clone().requires_grad_(True)
    gamma, beta = t["gamma"].clone().requires_grad_(True), t["beta"].clone().requires_grad_(True)
    emb = t["emb"].clone().requires_grad_(True) if c["film"] else None
    xg = x.view(B, HW, G, cg)
    # sum / n with n a tensor: a sum of integers is exact in any order and a true division correctly rounded, while .mean() and a
    # division by a Python number may multiply by 1 / n (seen on the GPU: 198 m / 198 != m, the exact regime's y off by 2^-50)
    n = torch.tensor(float(cg * HW), dtype=torch.float64, device=x.device)
    mean = xg.sum((1, 3)) / n
    var = (xg - mean[:, None, :, None]).pow(2).sum((1, 3)) / n
    rstd = 1.0 / torch.sqrt(var + c["eps"])
    xh = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, HW, C)
    n1 = xh * gamma + beta
    n2 = n1
    if c["film"]:
        sc, sh = _film(c, {"emb": emb})
        n2 = n1 * (1.0 + sc[:, None, :]) + sh[:, None, :]
    y = n2 * torch.sigmoid(n2) if c["silu"] else n2
    (y * t["dout"]).sum().backward()
    ref = {"mean": mean.detach(), "rstd": rstd.detach(), "y": y.detach(),
           "dx": x.grad + (t["dx_add"] if c["add"] else 0.0),
           "dgamma": gamma.grad + _old(c, t, "dgamma_old"), "dbeta": beta.grad + _old(c, t, "dbeta_old")}
    with torch.no_grad():
        s = torch.sigmoid(n2)
        dn2 = t["dout"] * (s * (1.0 + n2 * (1.0 - s))) if c["silu"] else t["dout"]
        dn1 = dn2
        if c["film"]:
            _, so, ho = film_layout(c)[:3]
            ref["dscale"], ref["dshift"] = emb.grad[:, so:so + C], emb.grad[:, ho:ho + C]
            dn1 = dn2 * (1.0 + sc[:, None, :])
        xgd = xg.detach()
        aux = {"dgamma": dn1 * xh, "dbeta": dn1, "dscale": dn2 * n1, "dshift": dn2, "absx": xgd.abs().mean((1, 3)), "x2": xgd.pow(2).mean((1, 3)),
               "var": var.detach()}
    return ref, aux


def _rms(v):
    return float(v.pow(2).mean().sqrt()) if v.numel() else 0.0


def stat_bounds(c, ref, aux):
    n = chain(c)
    bm = n * U * aux["absx"] + U * ref["mean"].abs()
    br = ref["rstd"] * (1.5 * n * U * aux["x2"] / (aux["var"] + c["eps"]) + 2.0 * U)
    return bm, br


def closed_form(c, t, mean, rstd):
    """The passes as the kernels form them from given statistics [B][G], in float64: y, dx, and the four per-(sample, channel) sums the
    backward reduces (A = sum dn1 xhat, Bs = sum dn1, DS = sum dn2 n1, DH = sum dn2).  With the reference's statistics this is the
    reference (test_gn_parity_cpu.py); stat_term() differences it."""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg = C // G
    mu, rs = _per_channel(mean, cg), _per_channel(rstd, cg)
    xh = (t["x"] - mu) * rs
    n1 = xh * t["gamma"] + t["beta"]
    sc, sh = _film(c, t)
    n2 = n1 * (1.0 + sc[:, None, :]) + sh[:, None, :] if c["film"] else n1
    s = torch.sigmoid(n2)
    y = n2 * s if c["silu"] else n2
    dn2 = t["dout"] * (s * (1.0 + n2 * (1.0 - s))) if c["silu"] else t["dout"]
    dn1 = dn2 * (1.0 + sc[:, None, :]) if c["film"] else dn2
    A, Bs, DS, DH = (dn1 * xh).sum(1), dn1.sum(1), (dn2 * n1).sum(1), dn2.sum(1)
    S1 = (t["gamma"] * Bs).view(B, G, cg).sum(2)
    S2 = (t["gamma"] * A).view(B, G, cg).sum(2)
    n = float(cg * HW)
    dx = rs * (dn1 * t["gamma"] - _per_channel(S1, cg) / n - xh * _per_channel(S2, cg) / n)
    if c["add"]:
        dx = dx + t["dx_add"]
    return {"y": y, "dx": dx, "A": A, "Bs": Bs, "DS": DS, "DH": DH}


def stat_term(c, t, ref, aux):
    """What the statistics bounds become in each output: the kernels compute every pass from the f32 mean and rstd of the forward, so
    an output o(mean, rstd) carries |do/dmean| bm + |do/drstd| br.  Taken as the larger of the two one-sided differences of
    closed_form() at the bounds themselves, per element (each element of y, dx, dscale and dshift depends on the statistics of its own
    (sample, group) only, so all groups are moved at once); dgamma and dbeta sum the per-sample differences in absolute value."""
    bm, br = stat_bounds(c, ref, aux)
    base = closed_form(c, t, ref["mean"], ref["rstd"])
    d = {k: torch.zeros_like(v) for k, v in base.items()}
    for dm, dr in ((bm, 0.0), (0.0, br)):
        hi, lo = closed_form(c, t, ref["mean"] + dm, ref["rstd"] + dr), closed_form(c, t, ref["mean"] - dm, ref["rstd"] - dr)
        for k in d:
            d[k] += torch.maximum((hi[k] - base[k]).abs(), (lo[k] - base[k]).abs())
    return {"y": d["y"], "dx": d["dx"], "dgamma": d["A"].sum(0), "dbeta": d["Bs"].sum(0), "dscale": d["DS"], "dshift": d["DH"]}


def evaluate(c, t):
    """-> (ref, bound): name -> float64 reference and per-element bound of every output of the case"""
    ref, aux = reference(c, t)
    bound = {}
    bound["mean"], bound["rstd"] = stat_bounds(c, ref, aux)
    for k in ("y", "dx"):
        r = ref[k]
        if c["dt"] == "f32":
            bound[k] = 1e-5 * r.abs() + 1e-5 * _rms(r)
        else:
            bound[k] = torch.pow(2.0, torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -120))) - 7) + 1e-5 * _rms(r)
    terms = {"dgamma": c["B"] * c["HW"], "dbeta": c["B"] * c["HW"], "dscale": c["HW"], "dshift": c["HW"]}
    for k, n in terms.items():
        if k in ref:
            bound[k] = 1e-5 * ref[k].abs() + 1e-5 * math.sqrt(n) * _rms(aux[k])
    if PROPAGATED:
        st = stat_term(c, t, ref, aux)
        for k in PROPAGATED:
            if k in bound:
                bound[k] = bound[k] + st[k]
    return ref, bound


def exact_outputs(c):
    """the outputs that must equal the reference (rounded to the output's format) in the exact regime"""
    if c["regime"] != "exact":
        return ()
    return OUTPUTS if exact_bwd(c) else ("mean", "rstd", "y")


def ratios(c, ref, bound, got):
    """name -> worst err / bound over the elements of each output; 0 / inf for equal / not equal where the exact regime asks for
    equality.  Every element counts; a NaN anywhere is inf."""
    assert set(got) == set(ref), (c["name"], sorted(got), sorted(ref))
    out, ex = {}, exact_outputs(c)
    for k, r in ref.items():
        gk = got[k].reshape(r.shape) if got[k].numel() == r.numel() else got[k]
        if gk.shape != r.shape or not bool(torch.isfinite(gk).all()):
            out[k] = float("inf")
        elif k in ex:
            out[k] = 0.0 if torch.equal(gk, rnd(r, c["dt"] if k in ("y", "dx") else "f32")) else float("inf")
        else:
            err, b = (gk - r).abs(), bound[k]
            q = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)),
                            torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            out[k] = float(q.max())
    return out


def reference_fits_f32(c, ref):
    """exact regime: the outputs asked to be equal are exactly representable in f32 (the regime's premise, without the kernels)"""
    return all(torch.equal(ref[k].float().double(), ref[k]) for k in exact_outputs(c) if k in ref)


# ------------------------------------------------------------------------------------------------------------------------------
# simulated kernels
# ------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("stats_next_group", "drop_last_row", "drop_chunk", "gamma_shift", "film_prev_sample", "s1_without_gamma", "dbeta_skip_b16",
          "drop_dx_add", "ignore_grad_beta", "silu_grad_sigmoid")
# the cases each fault is shown on (test_gn_parity_cpu.py asserts that the comparator flags it there)
FAULT_CASES = {
    "stats_next_group": ("quad_f32_1x3x4_g4_normal", "quad_bf16_1x1040x4_g4_exact", "flatf_3x129x136_g17_normal", "flatf_5x64x64_g64_exact"),
    "drop_last_row": ("quad_f32_17x1040x4_g1_offset", "quad_bf16_1x513x4_g1_exact", "flatf_3x129x136_g1_normal", "flat_512x16x8_g8_exact"),
    "drop_chunk": ("quad_f32_33x513x4_g4_normal", "quad_bf16_1x1040x4_g4_exact", "flatf_2x130x96_g32_normal", "flatf_3x129x136_g17_exact"),
    "gamma_shift": ("quad_f32_1x16x12_g1_normal", "quad_bf16_1x1x12_g3_exact", "flatf_2x40x1032_g24_normal", "flatf_3x129x136_g1_exact"),
    "film_prev_sample": ("quad_bf16_17x3x4_g1_normal", "quad_f32_33x16x4_g1_exact", "flatf_2x40x1032_g24_normal", "flat_512x16x8_g8_exact"),
    "s1_without_gamma": ("quad_f32_1x1x4_g1_normal", "quad_f32_33x16x4_g1_exact", "flatf_2x40x1032_g24_normal", "flat_512x16x8_g8_exact"),
    "dbeta_skip_b16": ("quad_bf16_17x16x4_g4_normal", "quad_f32_33x16x4_g1_exact", "flat_512x16x8_g8_normal", "flat_512x16x8_g8_exact"),
    "drop_dx_add": ("quad_f32_33x513x4_g4_normal", "quad_bf16_1x1040x4_g4_exact", "flatf_3x129x136_g1_normal", "flatf_5x64x64_g64_exact"),
    "ignore_grad_beta": ("quad_f32_1x3x4_g4_normal", "quad_bf16_17x16x4_g4_normal", "flatf_3x129x136_g1_exact", "flatf_3x129x136_g17_normal"),
    "silu_grad_sigmoid": ("quad_f32_1x16x12_g1_normal", "quad_f32_33x513x4_g4_normal", "flatf_3x129x136_g17_normal", "flatf_5x64x64_g64_normal"),
}


def fault_applies(c, fault):
    return {"stats_next_group": c["G"] > 1, "drop_last_row": True, "drop_chunk": c["target"]["nch"] > 1,
            "gamma_shift": c["C"] > (8 if c["target"]["variant"] == "flat" else 4), "film_prev_sample": bool(c["film"]) and c["B"] > 1,
            "s1_without_gamma": True, "dbeta_skip_b16": c["B"] > 16, "drop_dx_add": c["add"], "ignore_grad_beta": c["grad_beta"] != 1.0,
            "silu_grad_sigmoid": c["silu"]}[fault]


def _lane_sums(v, rows, lanes):
    """v [B][HW][C] f32 -> [nch][B][C]: per chunk of `rows` rows, every lane sums its rows (row i of a chunk: lane i % lanes), then
    the lanes are summed; all in f32"""
    B, HW, C = v.shape
    nch = -(-HW // rows)
    steps = -(-rows // lanes)
    p = torch.zeros(B, nch * rows, C, dtype=torch.float32)
    p[:, :HW] = v
    p = p.view(B, nch, rows, C)
    if steps * lanes > rows:
        p = torch.cat([p, torch.zeros(B, nch, steps * lanes - rows, C, dtype=torch.float32)], 2)
    return p.reshape(B, nch, steps, lanes, C).sum(2).sum(2).permute(1, 0, 2).contiguous()


def simulate(c, t, fault=None):
    """name -> float64 "kernel output" of the case made on the CPU in f32: the quad or the flat formulas on the planned chunks and
    lanes, sums folded as the group kernels fold them, outputs rounded to their storage format; `fault`: one of FAULTS"""
    assert fault is None or fault in FAULTS, fault
    f32 = torch.float32
    B, HW, C, G, dt = c["B"], c["HW"], c["C"], c["G"], c["dt"]
    cg, tg = C // G, c["target"]
    flat, rows = tg["variant"] == "flat", tg["rows"]
    lanes = tg["rpi"] if flat else 16
    x, dout = t["x"].to(f32), t["dout"].to(f32)
    gamma, beta = t["gamma"].to(f32), t["beta"].to(f32)
    sc, sh = _film(c, t)
    if c["film"]:
        sc, sh = sc.to(f32)[:, None, :], sh.to(f32)[:, None, :]
        if fault == "film_prev_sample":
            sc, sh = sc.roll(1, 0), sh.roll(1, 0)
    # ---- forward sums, statistics
    xs = x
    if fault == "drop_last_row":
        xs = x.clone()
        xs[:, [min((ch + 1) * rows, HW) - 1 for ch in range(tg["nch"])]] = 0.0
    ps, pq = _lane_sums(xs, rows, lanes), _lane_sums(xs * xs, rows, lanes)
    if fault == "drop_chunk":
        ps[-1], pq[-1] = 0.0, 0.0
    s, q = ps.double().sum(0).view(B, G, cg).sum(2), pq.double().sum(0).view(B, G, cg).sum(2)
    n = float(cg * HW)
    m = s / n
    var = (q / n - m * m).clamp_min(0.0)
    mean, rstd = m.to(f32), (1.0 / torch.sqrt(var + float(torch.tensor(c["eps"], dtype=f32)))).to(f32)
    use_m, use_r = (mean.roll(-1, 1), rstd.roll(-1, 1)) if fault == "stats_next_group" else (mean, rstd)
    mu, rs = _per_channel(use_m, cg), _per_channel(use_r, cg)
    ga = gamma.roll(-(8 if flat else 4)) if fault == "gamma_shift" else gamma
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    # ---- forward apply
    if flat:
        P, Q = rs * ga, beta - mu * rs * ga
        if c["film"]:
            P, Q = P * (1.0 + sc), Q * (1.0 + sc) + sh
        n2 = x * P + Q
    else:
        n2 = x * (rs * ga) + (beta - mu * rs * ga)
        if c["film"]:
            n2 = n2 * (1.0 + sc) + sh
    y = n2 * sig(n2) if c["silu"] else n2
    # ---- backward sums
    def act_grad(v):
        if not c["silu"]:
            return torch.ones_like(v)
        sg = sig(v)
        return sg if fault == "silu_grad_sigmoid" else sg * (1.0 + v * (1.0 - sg))
    one_sc = (1.0 + sc) if c["film"] else torch.ones(1, 1, 1, dtype=f32)
    if flat:
        d = dout * act_grad(x * P + Q)
        sd, sx = _lane_sums(d, rows, lanes), _lane_sums(d * (x - mu), rows, lanes)          # [nch][B][C]
        rs_c, s1 = rs[:, 0], one_sc[:, 0]
        parts = [s1 * (rs_c * sx), s1 * sd, gamma * (rs_c * sx) + beta * sd, sd]
        dn1 = None
    else:
        xh = (x - mu) * rs
        n1 = xh * ga + beta
        n2b = n1 * (1.0 + sc) + sh if c["film"] else n1
        dn2 = dout * act_grad(n2b)
        dn1 = dn2 * one_sc if c["film"] else dn2
        parts = [_lane_sums(v, rows, lanes) for v in (dn1 * xh, dn1, dn2 * n1, dn2)]
    A, Bs, DS, DH = (p.sum(0) for p in parts)                                                # fold the chunks: [B][C], f32
    S1 = ((Bs if fault == "s1_without_gamma" else gamma * Bs)).view(B, G, cg).sum(2)
    S2 = (gamma * A).view(B, G, cg).sum(2)
    gb = 1.0 if fault == "ignore_grad_beta" else c["grad_beta"]
    old = lambda k: gb * t[k].to(f32) if gb != 0.0 else torch.zeros(C, dtype=f32)
    dgamma = old("dgamma_old") + A.sum(0)
    dbeta = old("dbeta_old") + (Bs[:16] if fault == "dbeta_skip_b16" else Bs).sum(0)
    # ---- backward apply
    invn = torch.tensor(1.0, dtype=f32) / torch.tensor(float(cg) * HW, dtype=f32)
    S1c, S2c = _per_channel(S1 * invn, cg), _per_channel(S2 * invn, cg)
    if flat:
        K3 = rs * rs * S2c
        K2 = rs * S1c - K3 * mu
        dx = P * d - K3 * x - K2
    else:
        dx = rs * (dn1 * ga - S1c - xh * S2c)
    if c["add"] and fault != "drop_dx_add":
        dx = dx + t["dx_add"].to(f32)
    out = {"mean": mean.double(), "rstd": rstd.double(), "y": rnd(y, dt), "dx": rnd(dx, dt), "dgamma": dgamma.double(), "dbeta": dbeta.double()}
    if c["film"]:
        out["dscale"], out["dshift"] = DS.double(), DH.double()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the plan of a case
# ------------------------------------------------------------------------------------------------------------------------------
def describe_plan(c, p, L):
    """the fields of a planned pass a case declares, as a target dict"""
    last = c["HW"] - (p.nch - 1) * p.rows
    bg = c["B"] * c["G"]
    return dict(zip(TARGET_FIELDS, (("quad", "flat")[p.variant], p.rows, p.nch, p.nt, p.rpi, last, bg > 128, bg > 256)))


def plans_of(c, L, ops):
    """the four passes' targets under the case's switch (host arithmetic, no GPU); the switch is reset afterwards"""
    lib = L.lib()
    lib.vaw_debug_gn_flat(c["switch"])
    try:
        dt = L.F32 if c["dt"] == "f32" else L.BF16
        return [describe_plan(c, ops.gn_plan(p, dt, c["B"], c["HW"], c["C"], c["G"]), L)
                for p in (L.GN_FWD_SUMS, L.GN_APPLY, L.GN_BWD_SUMS, L.GN_BWD_APPLY)]
    finally:
        lib.vaw_debug_gn_flat(-1)

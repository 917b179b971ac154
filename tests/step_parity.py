"""Float64 references, error allowances and comparators for the objective kernels and the DiT conditioning / patch kernels of
csrc/elementwise.hip (q-sample and row mixes, weighted MSE and its batch mean, the variational-bound term, sinusoidal embedding, SiLU,
embedding lookup / scatter, the four patch shuffles, cast with column sums) and the vaw_reduce_rows fold of csrc/layernorm.hip.
Imported by test_step_kernels_cpu.py and test_gpu_step_kernels.py; no GPU needed, every reference lives on the CPU.

References.  Each is a plain float64 torch statement of the operation from the inputs the kernel is handed (f32 values widened to
float64).  A bf16 output is the f32 value rounded to nearest even (bf16_rne).

Comparators, three kinds:
  exact           torch.equal / same_bits: index shuffles, gathers, casts, and every reduction on small-integer inputs with power-of-two
                  coefficients, where each product is exact and each partial sum stays below 2^24 in any order.
  derived bound   f32 arithmetic on random data: (number of roundings) * 2^-24 * sum |terms|, computed in float64 from the same inputs;
                  the count is read from the kernel (the elementwise operations plus the longest chain of additions) and derived at the
                  function that computes it.  within() holds the kernel to it with no extra margin.
  transcendental  SiLU (__expf), the sinusoidal embedding (expf, cosf, sinf), the variational bound (expf, tanhf, logf): the float64
                  reference is the truth and the allowance per element is the larger of
                    (a) 4 x the error the same expression has when torch evaluates it in f32 on the CPU in the kernel's operation order
                        (the margin test_gpu_step_fused.py grants a reordered f32 computation), and
                    (b) a running error bound of the kernel's own operation sequence (class Run): every operation propagates the
                        absolute error of its operands to first order with the worst slope over the operand's error interval and adds
                        its own rounding, u = 2^-24 relative for + - * / and the accuracy the device function is defined with:
                          expf 3 ulp, logf 3 ulp, sinf / cosf 4 ulp, tanhf 5 ulp      (the OpenCL accuracy table the device library
                                                                                       follows; 1 ulp <= 2u |value|)
                          __expf(x) = exp2(fl(log2e_f32 * x)) by its definition in the compiler's HIP math header: log2e_f32 carries one
                              rounding and the product another, so the argument of exp2 is off by at most 2u |x log2e| and the result
                              by the factor 2^(2u |x| log2e) = e^(2u |x|) ~ 1 + 2u |x|; the exp2 instruction itself is good to 1 ulp =
                              2u and flushes results below 2^-126 to zero.  Relative error c0 + c1 |x| with c0 = c1 = 2u, plus 2^-126.
                        Nothing in (b) is fitted to what a kernel returns.
MEASURED: worst error / allowance per kernel on the MI355X (pytest -m gpu tests/test_gpu_step_kernels.py -s); also in DESIGN.md 5.4a."""
import math

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of f32
NAN = float("nan")
TAIL = 64                 # canary elements behind every output
CANARY = -7.0             # exact in bf16
F32_MAX = 3.4028234663852886e38
F32_TINY = 2.0 ** -126
LN2 = math.log(2.0)
SS_NCOEF = 16             # floats per row of the per-timestep table (csrc/elementwise.hip)

# worst error / allowance on the MI355X, by kernel (transcendental kind), from the -s output of the GPU file
MEASURED = {
    "vaw_silu_fwd": 0.91, "vaw_silu_bwd": 0.57, "vaw_timestep_embedding": 0.27, "vaw_vb_fwd": 0.037, "vaw_vb_bwd d_mean": 0.32,
    "vaw_vb_bwd d_var": 0.35,
}


# ------------------------------------------------------------------------------------------------------------------------------------
# buffers and bit comparators
# ------------------------------------------------------------------------------------------------------------------------------------
def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def ints(g, *shape, lo=-2, hi=2):
    """integers of [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def guarded(n, dtype, fill=NAN, device="cuda"):
    """n elements of `fill` (a number or a tensor of n values) with TAIL canary elements behind them"""
    buf = torch.full((n + TAIL,), CANARY, device=device, dtype=dtype)
    buf[:n] = fill
    return buf


def tail_intact(buf, n):
    return buf.numel() == n + TAIL and bool((buf[n:] == CANARY).all())


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def bf16_rne(x):
    """the bf16 value of an f32 (or float64 holding f32 values) tensor, round to nearest even: what from_f32<bf16_t> stores"""
    return x.float().to(torch.bfloat16)


def within(got, ref, allow):
    """derived bound, no margin: every element finite where the reference is, and |got - ref| <= allow.  Returns (ok, worst ratio)."""
    got, ref, allow = got.double(), ref.double(), allow.double()
    assert got.shape == ref.shape == allow.shape, (got.shape, ref.shape, allow.shape)
    err = (got - ref).abs()
    fin = torch.isfinite(ref)
    ok = bool(torch.isfinite(got[fin]).all()) and bool((err[fin] <= allow[fin]).all())
    ratio = err[fin] / allow[fin].clamp_min(1e-300)
    ratio = torch.where(err[fin] == 0, torch.zeros_like(ratio), ratio)
    return ok, float(ratio.max()) if ratio.numel() else 0.0


def transc_allow(ref64, cpu32, derived):
    """the transcendental allowance: max(4 |f32-on-the-CPU - float64|, derived running bound), elementwise"""
    e = (cpu32.double() - ref64).abs()
    e = torch.where(torch.isfinite(e), e, torch.zeros_like(e))
    return torch.maximum(4.0 * e, derived)


# ------------------------------------------------------------------------------------------------------------------------------------
# running error arithmetic: a float64 value with a bound on the absolute error of the f32 computation of it
# ------------------------------------------------------------------------------------------------------------------------------------
def _is_pow2(c):
    return c != 0 and math.frexp(abs(c))[0] == 0.5


def _f32_exact(c):
    return float(np.float32(c)) == float(c)


def _rounding(v, *operands):
    """u |v| for the rounding of an operation's result -- nothing where every operand is exact and so is the result (representable in
    f32): IEEE arithmetic returns it as it is"""
    exact = v.float().double() == v
    for o in operands:
        exact = exact & (o.e == 0)
    return torch.where(exact, torch.zeros_like(v), U * v.abs())


class Run:
    """v: the float64 value; e >= 0: a bound on |f32 result - v|.  Tensors as operands are exact inputs, python floats are constants
    (one rounding to f32 unless representable).  Every operation: first-order propagation of the operand errors (the second-order
    products included where they are cheap) plus one rounding u |result|; a product with a power of two rounds nothing."""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x, like=None):
        if isinstance(x, Run):
            return x
        if isinstance(x, torch.Tensor):
            return Run(x.double())
        v = torch.full_like(like.v, float(x)) if like is not None else torch.tensor(float(x), dtype=torch.float64)
        return Run(v, v.abs() * (0.0 if _f32_exact(x) else U))

    def __add__(self, o):
        o = Run.lift(o, self)
        v = self.v + o.v
        return Run(v, self.e + o.e + _rounding(v, self, o))

    __radd__ = __add__

    def __neg__(self):
        return Run(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Run.lift(o, self))

    def __rsub__(self, o):
        return Run.lift(o, self) + (-self)

    def __mul__(self, o):
        p2 = not isinstance(o, (Run, torch.Tensor)) and _is_pow2(float(o))
        o = Run.lift(o, self)
        v = self.v * o.v
        return Run(v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + (0.0 if p2 else 1.0) * _rounding(v, self, o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        p2 = not isinstance(o, (Run, torch.Tensor)) and _is_pow2(float(o))
        o = Run.lift(o, self)
        v = self.v / o.v
        den = o.v.abs() - o.e                                   # the smallest the divisor can be
        e = (self.e + v.abs() * o.e) / den
        e = torch.where(den > 0, e, torch.full_like(e, float("inf")))
        return Run(v, e + (0.0 if p2 else 1.0) * _rounding(v, self, o))

    def __rtruediv__(self, o):
        return Run.lift(o, self) / self

    def exp(self, ulps=3):
        v = torch.exp(self.v)
        return Run(v, v * torch.expm1(self.e) + ulps * 2 * U * v)

    def fast_exp(self):
        """__expf: see the module docstring -- relative 2u + 2u |x| on top of the propagated argument error, 2^-126 for the flush"""
        v = torch.exp(self.v)
        return Run(v, v * torch.expm1(self.e + 2 * U * self.v.abs()) + 2 * U * v + F32_TINY)

    def tanh(self, ulps=5):
        """The one assumption beyond the accuracy table: from |x| = 10 on, where the truth is within 2^-28 of +-1, tanhf returns +-1
        itself (the nearest f32, and what the CPU's f32 tanh gives): the 1e-12 floors of the decoder NLL are reached through it."""
        v = torch.tanh(self.v)
        near = (self.v.abs() - self.e).clamp_min(0.0)           # the point of the error interval with the steepest slope
        e = self.e * (1.0 - torch.tanh(near) ** 2) + ulps * 2 * U * v.abs()
        return Run(v, torch.where(near >= 10.0, torch.zeros_like(e), e))

    def log(self, ulps=3):
        v = torch.log(self.v)
        lo = self.v - self.e
        e = torch.where(lo > 0, self.e / lo.clamp_min(1e-300), torch.full_like(v, float("inf")))
        return Run(v, e + ulps * 2 * U * v.abs())

    def cos(self, ulps=4):
        v = torch.cos(self.v)
        return Run(v, self.e.clamp_max(2.0) + ulps * 2 * U * v.abs())       # |cos'| <= 1

    def sin(self, ulps=4):
        v = torch.sin(self.v)
        return Run(v, self.e.clamp_max(2.0) + ulps * 2 * U * v.abs())

    def clamp_min(self, m):
        return Run(self.v.clamp_min(m), torch.maximum(self.e, torch.full_like(self.e, U * abs(m))))   # 1-Lipschitz; m as an f32


class _TorchOps:
    """the functions of a restatement on plain tensors (float64: the truth; float32: the CPU comparison of the transcendental kind)"""
    exp = staticmethod(torch.exp)
    fast_exp = staticmethod(torch.exp)
    tanh = staticmethod(torch.tanh)
    log = staticmethod(torch.log)
    cos = staticmethod(torch.cos)
    sin = staticmethod(torch.sin)

    @staticmethod
    def clamp_min(x, m):
        return x.clamp(min=m)

    @staticmethod
    def where(c, a, b):
        return torch.where(c, a, b)

    @staticmethod
    def val(x):
        return x

    @staticmethod
    def zeros(like):
        return torch.zeros_like(like)


class _RunOps:
    exp = staticmethod(lambda x: x.exp())
    fast_exp = staticmethod(lambda x: x.fast_exp())
    tanh = staticmethod(lambda x: x.tanh())
    log = staticmethod(lambda x: x.log())
    cos = staticmethod(lambda x: x.cos())
    sin = staticmethod(lambda x: x.sin())

    @staticmethod
    def clamp_min(x, m):
        return x.clamp_min(m)

    @staticmethod
    def where(c, a, b):
        a, b = Run.lift(a), Run.lift(b)
        return Run(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))

    @staticmethod
    def val(x):
        return x.v

    @staticmethod
    def zeros(like):
        return Run(torch.zeros_like(like.v))


def _ops(x):
    return _RunOps if isinstance(x, Run) else _TorchOps


# ------------------------------------------------------------------------------------------------------------------------------------
# mix, q-sample, latent q-sample
# ------------------------------------------------------------------------------------------------------------------------------------
def gather_rows(tab, t):
    """tab[t[b]] as float64 [B]; NaN where t[b] is outside [0, len(tab)): the kernels poison such a row"""
    T = tab.numel()
    ok = (t >= 0) & (t < T)
    out = tab.double()[t.clamp(0, T - 1)]
    return torch.where(ok, out, torch.full_like(out, NAN))


def mix_ref(x, y, a, c):
    """out[b, :] = a[b] x[b, :] + c[b] y[b, :]; returns (float64 value, derived allowance).
    Allowance: two products and one sum, each rounded once (-ffp-contract=off): 3 roundings, none larger than u (|a x| + |c y|)."""
    x, y, a, c = x.double(), y.double(), a.double()[:, None], c.double()[:, None]
    return a * x + c * y, 3 * U * ((a * x).abs() + (c * y).abs())


def qsample_ref(x0, noise, t, tab_a, tab_s):
    """the timestep-gathered mix of vaw_qsample_fwd"""
    return mix_ref(x0, noise, gather_rows(tab_a, t), gather_rows(tab_s, t))


def latent_qsample_ref(latent, eps, noise, t, tab_a, tab_s, scale, t_scale):
    """latent [B, 2, n] (mean and std planes) -> x0 = (mean + std eps) scale, x_t = a x0 + c noise, tf = float(t) t_scale; scale and
    t_scale as the f32 values the kernel is handed.  Returns (x0, allow_x0, x_t, allow_xt, tf).
    Allowance: x0 takes a product, a sum and a product: 3 u (|mean| + |std eps|) |scale|.  x_t reads the rounded x0: |a| times that,
    plus its own 3 roundings."""
    scale, t_scale = float(np.float32(scale)), float(np.float32(t_scale))
    m, s = latent.double()[:, 0], latent.double()[:, 1]
    se = s * eps.double()
    x0 = (m + se) * scale
    a0 = 3 * U * (m.abs() + se.abs()) * abs(scale)
    a, c = gather_rows(tab_a, t)[:, None], gather_rows(tab_s, t)[:, None]
    xt = a * x0 + c * noise.double()
    at = a.abs() * a0 + 3 * U * ((a * x0).abs() + a.abs() * a0 + (c * noise.double()).abs())
    return x0, a0, xt, at, t.double() * t_scale


# ------------------------------------------------------------------------------------------------------------------------------------
# weighted MSE, its gradient, the batch mean
# ------------------------------------------------------------------------------------------------------------------------------------
def block_chain(items_per_thread, threads):
    """the longest chain of f32 additions a block reduction puts a value through: a thread's own items, 6 shuffle steps of the wave,
    the waves folded one after the other by block_sum"""
    return int(items_per_thread) + 6 + threads // 64


def wmse_ref(out, x0, noise, a, c, w):
    """mse[b] = w[b] mean((a[b] x0 + c[b] noise - out)^2); returns (value [B], derived allowance [B]).
    d = a x + c nz - o is four roundings of magnitudes <= S = |a x| + |c nz| + |o|: |delta d| <= 4 u S, so d^2 is off by 2 |d| 4 u S
    (+ u d^2 for the square).  The 1024 threads add their squares: ceil(n / 1024) items a thread on the scalar path; on the 16-byte
    path ceil(n / 4096) items of four squares, 4 additions each, at most ceil(n / 1024) + 3; then block_chain.  tot / n and w * that:
    two more roundings of the result."""
    n = out.shape[1]
    a, c, w = a.double()[:, None], c.double()[:, None], w.double()
    ax, cn, o = a * x0.double(), c * noise.double(), out.double()
    d = ax + cn - o
    S = ax.abs() + cn.abs() + o.abs()
    L = block_chain(-(-n // 1024) + 3, 1024)
    sq = (d * d).sum(1)
    allow = (2 * d.abs() * 4 * U * S + U * d * d).sum(1) + L * U * sq
    return w * sq / n, w.abs() * allow / n + 2 * U * (w * sq / n).abs()


def wmse_grad_ref(out, x0, noise, a, c, w, gm):
    """dout[b, :] = gm[b] w[b] 2 / n (out - a x0 - c noise); gm = g[b] (per-row form) or g * inv_count (scalar form: pass that product
    in float64).  Returns (value, allowance per rounding): the caller multiplies by its count --
    per-row form: k = gm w 2 / n is 2 roundings (the product with 2 is exact), the bracket a x, o - a x, c nz, - c nz is 4, k * it 1:
    7; the scalar form forms g * inv_count first: 8."""
    n = out.shape[1]
    a, c = a.double()[:, None], c.double()[:, None]
    k = (gm.double() * w.double() * 2.0 / n)[:, None]
    ax, cn, o = a * x0.double(), c * noise.double(), out.double()
    return k * (o - ax - cn), U * k.abs() * (o.abs() + ax.abs() + cn.abs())


def batch_mean_ref(v, accum):
    """out = (sum_b v[b]) / B / accum; returns (value, derived allowance): thread j of 256 adds v[j], v[j + 256], ...: ceil(B / 256)
    items, then block_chain; the two divisions round the result twice more."""
    B = v.numel()
    L = block_chain(-(-B // 256), 256)
    s = v.double().sum()
    return s / B / accum, (L + 2) * U * v.double().abs().sum() / B / accum


# ------------------------------------------------------------------------------------------------------------------------------------
# the variational-bound term: p_mean_variance and vb_elem of csrc/elementwise.hip in the kernel's operation order, generic over the
# arithmetic: float64 tensors (the truth; its gradients by autograd), float32 tensors, or Run (the running bound)
# ------------------------------------------------------------------------------------------------------------------------------------
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def p_mean_variance(c, mean_mode, var_mode, m, v, x_t):
    """c: the 16 table columns as [B, 1] tensors (exact inputs).  mean_mode 0: c2 pred + c3 x_t with pred = c0 x_t + c1 m; 1: m.
    var_mode 0: c5; 1: v; 2: frac c5 + (1 - frac) c4, frac = (v + 1) / 2.  Returns (mean, log variance)."""
    if var_mode == 1:
        lv = v
    elif var_mode == 2:
        frac = (v + 1.0) / 2.0
        lv = frac * c[5] + (1.0 - frac) * c[4]
    else:
        lv = c[5]
    if mean_mode == 1:
        return m, lv
    pred = x_t * c[0] + m * c[1]
    return pred * c[2] + x_t * c[3], lv


def vb_cdf(z):
    """0.5 (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3))) and its derivative in z, as the kernel writes them"""
    O = _ops(z)
    th = O.tanh(SQRT_2_OVER_PI * (z + 0.044715 * (z * z * z)))
    dcdf = 0.5 * (1.0 - th * th) * SQRT_2_OVER_PI * (1.0 + (3.0 * 0.044715) * z * z)
    return 0.5 * (1.0 + th), dcdf


def vb_elem(x0, true_mean, true_lv, mean, lv, t0, wrong_open_bins=False):
    """(val, d val / d lv, d val / d mean) per element, nats.  t0 [B, 1] bool: the decoder NLL of the row, otherwise the KL.
    x0 is an exact input (a tensor) and picks the bin.  wrong_open_bins: the named wrong answer of the CPU test, the middle bin's
    formula in the open-ended bins."""
    O = _ops(lv if isinstance(lv, Run) else mean)
    lift = (lambda q: Run.lift(q)) if O is _RunOps else (lambda q: q)
    mean, lv, true_mean, true_lv = lift(mean), lift(lv), lift(true_mean), lift(true_lv)
    # normal_kl
    e2, d, ratio = O.exp(-lv), true_mean - mean, O.exp(true_lv - lv)
    kl = 0.5 * (-1.0 + lv - true_lv + ratio + (d * d) * e2)
    kl_dlv = 0.5 * (1.0 - ratio - (d * d) * e2)
    kl_dmean = -d * e2
    # -discretized_gaussian_log_likelihood(x0; mean, 0.5 lv)
    cx, inv = lift(x0) - mean, O.exp(-(0.5 * lv))
    pin, mnn = inv * (cx + 1.0 / 255.0), inv * (cx - 1.0 / 255.0)
    cp, dp = vb_cdf(pin)
    cm, dm = vb_cdf(mnn)
    q, dl = 1.0 - cm, cp - cm
    lo, hi = x0 < -0.999, x0 > 0.999
    if wrong_open_bins:
        lo, hi = torch.zeros_like(lo), torch.zeros_like(hi)
    zero = O.zeros(cp)
    arg = O.where(lo, cp, O.where(hi, q, dl))
    live = O.val(arg) >= 1e-12                                  # below the floor the value is log(1e-12) and the gradient is zero
    lp = O.log(O.clamp_min(arg, 1e-12))
    safe = O.where(live, arg, zero + 1.0)
    g_pin = O.where(live & ~hi, dp / safe, zero)
    g_min = O.where(live & ~lo, -dm / safe, zero)
    nll, nll_dlv, nll_dmean = -lp, 0.5 * (g_pin * pin + g_min * mnn), inv * (g_pin + g_min)
    return O.where(t0, nll, kl), O.where(t0, nll_dlv, kl_dlv), O.where(t0, nll_dmean, kl_dmean)


def _vb_cols(coef, dtype):
    return [coef[:, i:i + 1].to(dtype) for i in range(SS_NCOEF)]


def vb_elements(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, dtype=torch.float64, run=False, **kw):
    """per-element (val, d_lv, d_mean) of a batch in `dtype`, or as Run values; coef [B, 16] f32 table rows"""
    c = _vb_cols(coef, torch.float64 if run else dtype)
    cast = (lambda q: None if q is None else q.double()) if run else (lambda q: None if q is None else q.to(dtype))
    m, v, x, z = cast(mean_out), cast(var_out), cast(x0), cast(xt)
    t0 = coef[:, 11:12] != 0
    if run:
        m, v, z = Run(m), (None if v is None else Run(v)), Run(z)
    mean, lv = p_mean_variance(c, mean_mode, var_mode, m, v, z)
    if run and not isinstance(lv, Run):
        lv = Run(lv.expand_as(x).clone())
    true_mean = (Run(x) if run else x) * c[2] + z * c[3]
    true_lv = c[4].expand_as(x)
    return vb_elem(x, true_mean, Run(true_lv.clone()) if run else true_lv, mean, lv, t0, **kw)


def vb_ref(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, scale, gvb=None, **kw):
    """float64: vb[b] = scale mean(val) / ln 2 and, given gvb [B], the gradients of sum_b gvb[b] vb[b] in mean_out and var_out by
    autograd (None where the mode does not read the tensor).  scale as the f32 value handed over."""
    scale = float(np.float32(scale))
    m = mean_out.double().clone().requires_grad_(gvb is not None)
    v = None if var_out is None else var_out.double().clone().requires_grad_(gvb is not None)
    val, _, _ = vb_elements(m, v, x0, xt, coef, mean_mode, var_mode, **kw)
    vb = scale * val.mean(1) / LN2
    if gvb is None:
        return vb.detach()
    ins = [m] + ([v] if v is not None and var_mode != 0 else [])
    grads = torch.autograd.grad((vb * gvb.double()).sum(), ins, allow_unused=True)
    dm = grads[0] if grads[0] is not None else torch.zeros_like(m)
    return vb.detach(), dm, (grads[1] if len(grads) > 1 else None)


def vb_fwd_allow(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, scale):
    """transcendental allowance of vaw_vb_fwd per row: (a) 4 x the f32-on-the-CPU error of the same per-row mean; (b) the running
    bound of every element's value, summed, plus the summation chain of the 1024 threads (block_chain(ceil(n / 1024))) and the
    three roundings of tot / n / ln2_f32 * scale with ln2_f32's own.  Returns (allowance [B], sum |val| [B])."""
    n, scale = x0.shape[1], float(np.float32(scale))
    ref = vb_ref(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, scale)
    v32, _, _ = vb_elements(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, dtype=torch.float32)
    cpu32 = scale * ((v32.sum(1) / float(n)) / float(np.float32(LN2)))
    r, _, _ = vb_elements(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, run=True)
    mag = r.v.abs().sum(1)
    L = block_chain(-(-n // 1024), 1024)
    derived = abs(scale) / (n * LN2) * (r.e.sum(1) + (L + 4) * U * mag)
    return transc_allow(ref, cpu32, derived), mag


def vb_bwd_allow(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, scale, gvb):
    """transcendental allowances of vaw_vb_bwd's (d_mean, d_var): g = gvb scale / (n ln2_f32) is 3 roundings and the constant's,
    the chain-rule factor (c2 * c1, or 0.5 (c5 - c4)) one, the two products g * d * factor two: 7 u |result| on top of g factor
    times the element's running bound."""
    n, scale = x0.shape[1], float(np.float32(scale))
    _, dm_ref, dv_ref = vb_ref(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, scale, gvb=gvb)
    c64, c32 = coef.double(), coef.float()
    out = []
    _, dlv32, dmean32 = vb_elements(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, dtype=torch.float32)
    r = vb_elements(mean_out, var_out, x0, xt, coef, mean_mode, var_mode, run=True)
    g64 = (gvb.double() * scale / (n * LN2))[:, None]
    g32 = ((gvb.float() * scale) / float(np.float32(n) * np.float32(LN2)))[:, None]
    for ref, e32, rr, f64, f32 in (
            (dm_ref, dmean32, r[2], (c64[:, 2] * c64[:, 1]) if mean_mode == 0 else torch.ones(len(c64), dtype=torch.float64),
             (c32[:, 2] * c32[:, 1]) if mean_mode == 0 else torch.ones(len(c32))),
            (dv_ref, dlv32, r[1], 0.5 * (c64[:, 5] - c64[:, 4]) if var_mode == 2 else torch.ones(len(c64), dtype=torch.float64),
             0.5 * (c32[:, 5] - c32[:, 4]) if var_mode == 2 else torch.ones(len(c32)))):
        if ref is None:
            out.append((None, None))
            continue
        cpu32 = g32 * e32 * f32[:, None]
        derived = (g64 * f64[:, None]).abs() * rr.e + 7 * U * (g64 * rr.v * f64[:, None]).abs()
        out.append((ref, transc_allow(ref, cpu32, derived)))
    return out


def table_rows(diff, mean_mode, var_kind):
    """[T, 16] f32 rows of the per-timestep table from an oracle GaussianDiffusion's float64 arrays, the columns vaw_vb_fwd reads
    (layout above SS_NCOEF in csrc/elementwise.hip): mean_mode 0 EPSILON (pa = sqrt(1 / abar), pb = -sqrt(1 / abar - 1)), 1 PREVIOUS_X;
    var_kind "large" / "small" (fixed) or "learned" (column 5 = log beta, the upper end of the learned range)."""
    f = lambda arr: torch.from_numpy(np.asarray(arr, dtype=np.float64)).float()
    T = diff.num_timesteps
    lv_aux = {"large": np.log(np.append(diff.posterior_variance[1], diff.betas[1:])), "small": diff.posterior_log_variance_clipped,
              "learned": np.log(diff.betas)}[var_kind]
    rows = torch.zeros(T, SS_NCOEF)
    rows[:, 0], rows[:, 1] = f(diff.sqrt_recip_alphas_cumprod), -f(diff.sqrt_recipm1_alphas_cumprod)
    if mean_mode == 1:
        rows[:, 0], rows[:, 1] = -f(diff.posterior_mean_coef2 / diff.posterior_mean_coef1), f(1.0 / diff.posterior_mean_coef1)
    rows[:, 2], rows[:, 3] = f(diff.posterior_mean_coef1), f(diff.posterior_mean_coef2)
    rows[:, 4], rows[:, 5] = f(diff.posterior_log_variance_clipped), f(lv_aux)
    rows[0, 11] = 1.0
    return rows


# ------------------------------------------------------------------------------------------------------------------------------------
# sinusoidal embedding, SiLU
# ------------------------------------------------------------------------------------------------------------------------------------
def _embedding(t, dim, nl, cast):
    """[B, dim]: cos(t f_i) | sin(t f_i) | one zero column if dim is odd, f_i = exp(nl i / half), in the kernel's operation order"""
    half = dim // 2
    B = t.shape[0]
    i = cast(torch.arange(half, dtype=torch.float64)[None, :].expand(B, half))
    if half == 0:
        return None
    arg = i * nl / float(half)
    O = _ops(arg)
    ang = O.exp(arg) * t
    return O.cos(ang), O.sin(ang)


def timestep_embedding_ref(t, dim, max_period=10000.0):
    """float64 embedding of f32 timesteps t [B]; returns (value [B, dim], transcendental allowance [B, dim]).  The kernel is handed
    -logf(max_period) as an f32: one rounding of the constant (a python float in the running bound), then nl * i, / half, expf, t * f
    and cosf / sinf, each as Run charges them; the angle's error enters cos and sin with slope <= 1."""
    B, half = t.numel(), dim // 2
    ref, allow = torch.zeros(B, dim, dtype=torch.float64), torch.zeros(B, dim, dtype=torch.float64)
    if half:
        t64 = t.double()[:, None].expand(B, half)
        nl = -math.log(max_period)
        c64, s64 = _embedding(t64, dim, nl, lambda q: q)
        nl32 = float(np.float32(nl))
        c32, s32 = _embedding(t.float()[:, None].expand(B, half), dim, nl32, lambda q: q.float())
        rc, rs = _embedding(t64, dim, nl, Run)
        ref[:, :half], ref[:, half:2 * half] = c64, s64
        allow[:, :half], allow[:, half:2 * half] = transc_allow(c64, c32, rc.e), transc_allow(s64, s32, rs.e)
    return ref, allow


def _silu(x):
    """x / (1 + __expf(-x)) and s (1 + x (1 - s)), s = 1 / (1 + __expf(-x)): silu_f and silu_grad_f of csrc/common.h"""
    O = _ops(x)
    E = O.fast_exp(-x)
    s = 1.0 / (1.0 + E)
    return x / (1.0 + E), s * (1.0 + x * (1.0 - s))


SILU_RUN_MAX = 87.0       # beyond it e^|x| leaves f32 and the running bound has nothing finite to say: allowance (a) alone


def silu_ref(x, dy=None):
    """float64 SiLU of f32 x and (given dy) dy * SiLU'(x); returns [(value, transcendental allowance)] for the forward and, with dy,
    the backward.  The running bound follows _silu operation by operation with __expf charged 2u + 2u |x| (module docstring); for
    |x| > 87, where __expf(-x) overflows to inf (the quotient is then a signed zero, the truth within 1e-36 of it) it is left out."""
    x64 = x.double()
    f64, g64 = _silu(x64)
    f32, g32 = _silu(x.float())
    inside = x64.abs() <= SILU_RUN_MAX
    rf, rg = _silu(Run(torch.where(inside, x64, torch.zeros_like(x64))))
    zero = torch.zeros_like(x64)
    out = [(f64, transc_allow(f64, f32, torch.where(inside, rf.e, zero)))]
    if dy is not None:
        d64 = dy.double()
        derived = d64.abs() * rg.e + U * (d64 * rg.v).abs()             # the product dy * grad: one more rounding
        out.append((d64 * g64, transc_allow(d64 * g64, dy.float() * g32, torch.where(inside, derived, zero))))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# embedding lookup and scatter
# ------------------------------------------------------------------------------------------------------------------------------------
def add_embedding_ref(a, table, idx):
    """out[b, :] = a[b, :] + table[idx[b], :] in float64; a row whose index is outside [0, rows) is NaN.  One f32 addition: the f32
    rounding of this value is the kernel's result bit for bit (exact kind)."""
    rows = table.shape[0]
    ok = (idx >= 0) & (idx < rows)
    out = a.double() + table.double()[idx.clamp(0, rows - 1)]
    out[~ok] = NAN
    return out


def embedding_bwd_ref(dc, idx, dtable, beta, reverse=False):
    """dtable[r, :] = beta dtable[r, :] + sum over {b : idx[b] == r} dc[b, :], b ascending, in the dtype of dc: float64 for the exact
    integer cases, float32 for the bitwise statement of the promised order (one accumulator from 0, rows added one by one, then
    (beta != 0 ? beta * old : 0) + acc).  Indices outside [0, rows) are ignored; beta = 0 does not read the table.
    reverse: the named wrong answer of the CPU test."""
    rows, D = dtable.shape
    acc = torch.zeros(rows, D, dtype=dc.dtype)
    order = range(dc.shape[0] - 1, -1, -1) if reverse else range(dc.shape[0])
    for b in order:
        r = int(idx[b])
        if 0 <= r < rows:
            acc[r] += dc[b]
    if beta == 0.0:
        return acc
    return torch.tensor(beta, dtype=dc.dtype) * dtable.to(dc.dtype) + acc


# ------------------------------------------------------------------------------------------------------------------------------------
# patch shuffles
# ------------------------------------------------------------------------------------------------------------------------------------
def patchify_ref(img, p):
    """[B, C, H, W] -> [B, (H/p)(W/p), C p p], column k = (c p + i) p + j: the Conv2d(kernel = stride = p) operand, by unfold"""
    return torch.nn.functional.unfold(img, kernel_size=p, stride=p).transpose(1, 2).contiguous()


def patchify_bwd_ref(dtok, C, H, W, p):
    """the transpose of patchify_ref (a permutation: its inverse), by fold"""
    return torch.nn.functional.fold(dtok.transpose(1, 2), (H, W), kernel_size=p, stride=p)


def unpatchify_ref(tok, C, H, W, p):
    """[B, (H/p)(W/p), p p C] with column k = (i p + j) C + c -> [B, C, H, W]: einsum nhwpqc->nchpwq"""
    B = tok.shape[0]
    return torch.einsum("nhwpqc->nchpwq", tok.reshape(B, H // p, W // p, p, p, C)).reshape(B, C, H, W)


def unpatchify_bwd_ref(dimg, p):
    B, C, H, W = dimg.shape
    return torch.einsum("nchpwq->nhwpqc", dimg.reshape(B, C, H // p, p, W // p, p)).reshape(B, (H // p) * (W // p), p * p * C)


# ------------------------------------------------------------------------------------------------------------------------------------
# cast with column sums, the row fold
# ------------------------------------------------------------------------------------------------------------------------------------
def cast_colsum_ref(src, colsum, beta):
    """dst = bf16(src) (nearest even); colsum[n] = beta colsum[n] + sum_m float(dst[m, n]) in float64: the sums of the values as stored"""
    dst = bf16_rne(src)
    s = dst.double().sum(0)
    return dst, (s if beta == 0.0 else beta * colsum.double() + s)


def reduce_rows_ref(partial, out, beta):
    """out[c] = beta out[c] + sum_r partial[r, c]; returns (value, derived allowance): 32 row groups add rows g, g + 32, ...:
    ceil(R / 32) additions, the 32 group sums are folded one after the other: 32 more, then beta * out and the final sum: 2."""
    R = partial.shape[0]
    s = partial.double().sum(0)
    mag = partial.double().abs().sum(0)
    if beta == 0.0:
        return s, (-(-R // 32) + 32 + 2) * U * mag
    return beta * out.double() + s, (-(-R // 32) + 32 + 2) * U * (mag + (beta * out.double()).abs())


# ------------------------------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU checks (allowance against result) and the GPU tests
# ------------------------------------------------------------------------------------------------------------------------------------
T_STEPS = 1000


def mse_case(B, n, integer, seed=0):
    """inputs of the row streams and the weighted MSE: out / x0 / noise [B, n] f32, tables ca / cb / w [T] f32.  integer: data in
    [-2, 2] and power-of-two tables (|ca|, |cb| in {0.5, 1, 2}, w in {0.5, 1, 2, 4}), so that a x + c nz - o is a multiple of 0.5 of
    magnitude <= 10 and every sum of squares a multiple of 0.25 below 100 n <= 1.3e6 < 2^22: exact in f32 in any order."""
    g = gen(B, n, int(integer), seed, 101)
    if integer:
        o, x, z = (ints(g, B, n).float() for _ in range(3))
        pw = lambda lo, hi: 2.0 ** torch.randint(lo, hi + 1, (T_STEPS,), generator=g).float()
        sign = lambda: torch.randint(0, 2, (T_STEPS,), generator=g).float() * 2 - 1
        ca, cb, w = pw(-1, 1) * sign(), pw(-1, 1) * sign(), pw(-1, 2)
    else:
        o, x, z = (torch.randn(B, n, generator=g) for _ in range(3))
        ca, cb, w = (lo + (hi - lo) * torch.rand(T_STEPS, generator=g) for lo, hi in ((0.5, 1.0), (0.1, 1.0), (0.5, 2.0)))
    return dict(out=o, x0=x, noise=z, ca=ca, cb=cb, w=w)


def timesteps(B, seed=0):
    """[B] int64 in [0, T): 0 and T - 1 first, the rest seeded"""
    t = torch.randint(0, T_STEPS, (B,), generator=gen(B, seed, 103))
    t[0] = 0
    if B > 1:
        t[1] = T_STEPS - 1
    return t


def reduce_case(R, N, integer, seed=0):
    """partial rows [R, N] and the previous out [N].  integer: [-2, 2], a column sums to at most 2 R + 2 <= 2002 in magnitude.
    random: 1 + N(0, 1) / 4, so that no column cancels and the allowance stays a small fraction of the result."""
    g = gen(R, N, int(integer), seed, 107)
    if integer:
        return ints(g, R, N).float(), ints(g, N).float()
    return 1.0 + 0.25 * torch.randn(R, N, generator=g), 1.0 + 0.25 * torch.randn(N, generator=g)


_DIFF = {}


def oracle_diffusion():
    """the oracle's float64 schedule arrays (linear betas, T = 1000)"""
    if "d" not in _DIFF:
        from types import SimpleNamespace

        from oracle import diffusion as od
        args = SimpleNamespace(weight_type="lambda", gamma=0.0, learn_sigma=False, p2_gamma=1, p2_k=1)
        _DIFF["d"] = od.GaussianDiffusion(args=args, betas=od.get_named_beta_schedule("linear", T_STEPS),
                                          model_mean_type=od.ModelMeanType.EPSILON, model_var_type=od.ModelVarType.FIXED_LARGE,
                                          loss_type=od.LossType.MSE)
    return _DIFF["d"]


VB_T = (0, 500, 999)      # the rows of a vb case: the decoder NLL row, two KL rows
VB_MODES = [(mm, vm) for mm in (0, 1) for vm in (0, 1, 2)]
VB_FLOORS = 3             # elements at the head of each bin of the t = 0 row that drive the bin's 1e-12 floor


def vb_bins(n):
    """index ranges of the t = 0 row: x0 = -1 (the open bin below -0.999), x0 = +1 (the open bin above 0.999), the rest inside"""
    k = max(n // 3, 1)
    return slice(0, k), slice(k, 2 * k), slice(2 * k, n)


def vb_case(n, mean_mode, var_mode, seed=0):
    """B = 3 rows at t = VB_T of the linear schedule: x0, x_t = q_sample(x0), the model's mean output up to 1.5 posterior standard deviations
    (uniformly) off the true posterior mean -- so that the KL and NLL elements are O(1), no row's value is a cancelled remainder and
    no bin's probability falls to where 1 + tanh has cancelled its f32 digits away (below 0.1) -- and its variance values (var_mode 1: the true log variance + 0.3 N(0, 1); 2: uniform in [-0.9, 0.9]).  Row 0 has
    x0 = -1, +1 and U(-0.9, 0.9) by vb_bins, and the first VB_FLOORS elements of each bin have the model mean half a unit (dozens
    of standard deviations) on the side that drives the bin's probability to zero: cdf_plus (low bin), 1 - cdf_min (high bin),
    cdf_plus - cdf_min (inside)."""
    d = oracle_diffusion()
    g = gen(n, mean_mode, var_mode, seed, 109)
    B = len(VB_T)
    t = torch.tensor(VB_T)
    coef = table_rows(d, mean_mode, "large" if var_mode == 0 else "learned")[t]
    x0 = (torch.rand(B, n, generator=g) * 1.8 - 0.9)
    lo, hi, mid = vb_bins(n)
    x0[0, lo], x0[0, hi] = -1.0, 1.0
    noise = torch.randn(B, n, generator=g)
    f = lambda arr: torch.from_numpy(np.asarray(arr)).float()[t][:, None]
    xt = f(d.sqrt_alphas_cumprod) * x0 + f(d.sqrt_one_minus_alphas_cumprod) * noise
    c = coef.double()
    std = torch.exp(0.5 * c[:, 4:5])
    target = c[:, 2:3] * x0.double() + c[:, 3:4] * xt.double() + 1.5 * std * (2.0 * torch.rand(B, n, generator=g).double() - 1.0)   # the model's mean
    target[:, -1] = (c[:, 2:3] * x0.double() + c[:, 3:4] * xt.double() + 1.5 * std)[:, -1]   # an O(1) last element: dropping it shows
    for sl, side in ((lo, 0.5), (hi, -0.5), (mid, 0.5)):
        idx = torch.arange(n)[sl][:VB_FLOORS]
        target[0, idx] = x0[0, idx].double() + side
    if mean_mode == 1:
        m = target
    else:                                                        # mean = c2 (c0 x_t + c1 m) + c3 x_t
        m = ((target - c[:, 3:4] * xt.double()) / c[:, 2:3] - c[:, 0:1] * xt.double()) / c[:, 1:2]
    v = None
    if var_mode == 1:
        v = (c[:, 4:5] + 0.3 * torch.randn(B, n, generator=g).double()).float()
    elif var_mode == 2:
        v = torch.rand(B, n, generator=g) * 1.8 - 0.9
    gvb = 0.5 + torch.rand(B, generator=g)
    floors = torch.cat([torch.arange(n)[sl][:VB_FLOORS] for sl in (lo, hi, mid)])
    return dict(mean_out=m.float(), var_out=v, x0=x0, xt=xt, coef=coef, gvb=gvb, scale=0.75, floors=floors)

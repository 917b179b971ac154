// HBM-bound kernels of the diffusion objective and the optimizer: q_sample, weighted MSE,
// sinusoidal embedding, SiLU, embedding gather/scatter, patchify/unpatchify, AdamW+EMA.
// All are coalesced 16-byte streams (float4 / bf16x4), grid-strided, capped at 8 blocks per CU.
#include "common.h"

static inline int stream_grid(int64_t work_items, int block) {
    int64_t g = (work_items + block - 1) / block;
    const int64_t cap = 256 * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---------------------------------------------------------------------------------------------
// out[b,:] = ca[b]*x[b,:] + cb[b]*y[b,:]; coefficients either given per row or gathered from tables.
// ---------------------------------------------------------------------------------------------
// the two coefficients of row b gathered from their tables at t[b]; t out of [0, T) poisons the row with NaN
__device__ __forceinline__ void gather_mix_coef(const float* __restrict__ ca, const float* __restrict__ cb, const int64_t* __restrict__ t,
                                                int T, int b, float& a, float& c) {
    const int64_t tt = t[b];
    const bool ok = tt >= 0 && tt < T;
    a = ok ? ca[tt] : __builtin_nanf("");
    c = ok ? cb[tt] : __builtin_nanf("");
}

template <bool GATHER>
__global__ void mix_rows_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ ca,
                                const float* __restrict__ cb, const int64_t* __restrict__ t, int T,
                                float* __restrict__ out, int64_t n, int vec4) {
    const int b = blockIdx.y;
    float a, c;
    if (GATHER) {
        gather_mix_coef(ca, cb, t, T, b, a, c);
    } else {
        a = ca[b];
        c = cb[b];
    }
    const float* xr = x + (int64_t)b * n;
    const float* yr = y + (int64_t)b * n;
    float* orow = out + (int64_t)b * n;
    const int64_t n4 = vec4 ? n / 4 : 0;                      // the host's vec4_ok: n % 4 == 0 and every pointer 16-byte aligned
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 xv = load4(xr + 4 * i), yv = load4(yr + 4 * i);
        store4(orow + 4 * i, a * xv + c * yv);
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        orow[i] = a * xr[i] + c * yr[i];
}

extern "C" int vaw_qsample_fwd(const float* x0, const float* noise, const int64_t* t, const float* tab_a,
                               const float* tab_s, int num_timesteps, float* x_t, int B, int64_t per_sample,
                               vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0 && num_timesteps > 0, "qsample: bad sizes B=%d n=%ld", B, (long)per_sample);
    int gx = stream_grid(per_sample / 4 + 1, 256);
    dim3 grid(gx > 64 ? 64 : gx, B);
    mix_rows_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(x0, noise, tab_a, tab_s, t, num_timesteps, x_t, per_sample,
                                                                 vec4_ok(per_sample, 0, {x0, noise, x_t}));
    VAW_CHECK_LAUNCH("qsample");
    return VAW_OK;
}

extern "C" int vaw_mix_rows(const float* x, const float* y, const float* ca, const float* cb, float* out, int B,
                            int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "mix_rows: bad sizes");
    int gx = stream_grid(per_sample / 4 + 1, 256);
    dim3 grid(gx > 64 ? 64 : gx, B);
    mix_rows_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, y, ca, cb, nullptr, 0, out, per_sample, vec4_ok(per_sample, 0, {x, y, out}));
    VAW_CHECK_LAUNCH("mix_rows");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Weighted MSE: one block per sample; wave shuffles + one LDS hop for the reduction.  One pair of kernels serves the per-row
// coefficient vectors of vaw_wmse_fwd / _bwd and the in-kernel table gather of vaw_wmse_fwd_t / _bwd_t.
// ---------------------------------------------------------------------------------------------
// Weighted MSE with its coefficients gathered inside: row b reads ca / cb / w at t[b] (t == NULL: at b, the per-row vectors of
// vaw_wmse_fwd -- the flow-matching objective has no tables).  t out of [0, T) poisons the row with NaN, as vaw_qsample_fwd does.
struct WmseCoef { float a, c, w; };
__device__ __forceinline__ WmseCoef wmse_coef(const float* ca, const float* cb, const float* w, const int64_t* t, int T, int b) {
    if (!t) return WmseCoef{ca[b], cb[b], w[b]};
    const int64_t tt = t[b];
    const float nan = __builtin_nanf("");
    return (tt >= 0 && tt < T) ? WmseCoef{ca[tt], cb[tt], w[tt]} : WmseCoef{nan, nan, nan};
}
__global__ void wmse_fwd_t_kernel(const float* __restrict__ o, const float* __restrict__ x0, const float* __restrict__ nz,
                                  const float* __restrict__ ca, const float* __restrict__ cb, const float* __restrict__ w,
                                  const int64_t* __restrict__ t, int T, float* __restrict__ mse, int64_t n, int vec4) {
    __shared__ float scratch[16];
    const int b = blockIdx.x;
    const WmseCoef k = wmse_coef(ca, cb, w, t, T, b);
    const float a = k.a, c = k.c;
    const float* orow = o + (int64_t)b * n;
    const float* xr = x0 + (int64_t)b * n;
    const float* nr = nz + (int64_t)b * n;
    float acc = 0.f;
    const int64_t n4 = vec4 ? n / 4 : 0;
    for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
        f32x4 d = a * load4(xr + 4 * i) + c * load4(nr + 4 * i) - load4(orow + 4 * i);
        acc += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
    }
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
        float d = a * xr[i] + c * nr[i] - orow[i];
        acc += d * d;
    }
    float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) mse[b] = k.w * (tot / (float)n);
}
// the gradient of sum_b gm[b] * mse[b].  g_per_row: gm = g[b], the vector autograd hands vaw_wmse_bwd.  Otherwise g is the device
// scalar handed down for the batch mean (1 for the loss itself) and inv_count = 1 / (B * accumulation steps): g * inv_count is the
// gmse[b] the mean's backward would have expanded
__global__ void wmse_bwd_t_kernel(const float* __restrict__ o, const float* __restrict__ x0, const float* __restrict__ nz,
                                  const float* __restrict__ ca, const float* __restrict__ cb, const float* __restrict__ w,
                                  const int64_t* __restrict__ t, int T, const float* __restrict__ g, int g_per_row, float inv_count,
                                  float* __restrict__ dout, int64_t n, int vec4) {
    const int b = blockIdx.y;
    const WmseCoef kc = wmse_coef(ca, cb, w, t, T, b);
    const float a = kc.a, c = kc.c;
    const float gm = g_per_row ? g[b] : g[0] * inv_count;
    const float k = gm * kc.w * 2.f / (float)n;
    const float* orow = o + (int64_t)b * n;
    const float* xr = x0 + (int64_t)b * n;
    const float* nr = nz + (int64_t)b * n;
    float* dr = dout + (int64_t)b * n;
    const int64_t n4 = vec4 ? n / 4 : 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        store4(dr + 4 * i, k * (load4(orow + 4 * i) - a * load4(xr + 4 * i) - c * load4(nr + 4 * i)));
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dr[i] = k * (orow[i] - a * xr[i] - c * nr[i]);
}
// out[0] = (sum_b v[b]) / B / accum in one fixed order: thread j adds v[j], v[j + 256], ... ascending, then block_sum's tree
__global__ void __launch_bounds__(256) batch_mean_kernel(const float* __restrict__ v, int B, float accum, float* __restrict__ out) {
    __shared__ float scratch[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) acc += v[i];
    const float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) out[0] = (tot / (float)B) / accum;
}

extern "C" int vaw_wmse_fwd(const float* model_out, const float* x0, const float* noise, const float* ca,
                            const float* cb, const float* w, float* mse, int B, int64_t per_sample,
                            vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "wmse_fwd: bad sizes");
    wmse_fwd_t_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(model_out, x0, noise, ca, cb, w, nullptr, 0, mse, per_sample,
                                                           vec4_ok(per_sample, 0, {model_out, x0, noise}));
    VAW_CHECK_LAUNCH("wmse_fwd");
    return VAW_OK;
}

extern "C" int vaw_wmse_bwd(const float* model_out, const float* x0, const float* noise, const float* ca,
                            const float* cb, const float* w, const float* gmse, float* dout, int B,
                            int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "wmse_bwd: bad sizes");
    int gx = stream_grid(per_sample / 4 + 1, 256);
    dim3 grid(gx > 64 ? 64 : gx, B);
    wmse_bwd_t_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(model_out, x0, noise, ca, cb, w, nullptr, 0, gmse, 1, 1.f, dout, per_sample,
                                                            vec4_ok(per_sample, 0, {model_out, x0, noise, dout}));
    VAW_CHECK_LAUNCH("wmse_bwd");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// The per-timestep table of the reverse process and its per-element p_mean_variance (reference :278-384), shared by the
// variational-bound term of the training loss, the likelihood evaluation and the reverse step.
// One row of SS_NCOEF floats per timestep (GaussianDiffusion._sample_table: the reference's f64 tables cast to f32):
//    0 pa, 1 pb     pred_xstart = pa*x_t + pb*mean_out (clamped to [-1,1] if clip)
//    2 c1, 3 c2     posterior mean coefficients: q mean = c1*x0 + c2*x_t, model mean = c1*pred + c2*x_t
//    4 plv          clipped posterior log variance (true log variance; lower end of the learned range)
//    5 lv_aux       the fixed model log variance, or log(beta_t), the upper end of the learned range
//    6 ra, 7 rm1    eps = (ra*x_t - pred)/rm1
//    8 sqrt_abp, 9 s1, 10 abp, 12 s2    ddim: sigma = (eta*s1)*s2, mean = pred*sqrt_abp + sqrt(1 - abp - sigma^2)*eps
//   11 is_t0        t == 0: no noise added; decoder NLL instead of the KL
//   13 abn          alphas_cumprod_next (DDIM reverse step)        14, 15 unused
//   mean_mode 0: model mean = c1*pred + c2*x_t      1: model mean = mean_out (PREVIOUS_X)
//   var_mode  0: log variance = lv_aux (fixed)   1: = var values (LEARNED)   2: interpolated (LEARNED_RANGE)
// ---------------------------------------------------------------------------------------------
#define SS_NCOEF 16
struct Pmv { float pred, mean, lv; };
// m / v: the model's mean output and variance value of the element (v is not read with a fixed variance), x_t the noised image
__device__ __forceinline__ Pmv p_mean_variance(const float* c, int mean_mode, int var_mode, int clip, float m, float v, float x_t) {
    Pmv o;
    float pred = c[0] * x_t + c[1] * m;
    if (clip) pred = fminf(fmaxf(pred, -1.f), 1.f);
    if (var_mode == 1) o.lv = v;
    else if (var_mode == 2) { const float frac = (v + 1.f) / 2.f; o.lv = frac * c[5] + (1.f - frac) * c[4]; }
    else o.lv = c[5];
    o.pred = pred;
    o.mean = mean_mode == 1 ? m : c[2] * pred + c[3] * x_t;
    return o;
}

// ---------------------------------------------------------------------------------------------
// Variational-bound term (learned variance / KL losses): one pass over (x0, x_t, model mean, model var values) per
// sample, bits per dim.  coef[b] is the table row of t[b]; no clipping.
// ---------------------------------------------------------------------------------------------
struct VbElem {
    float val;      // KL or decoder NLL of this element, nats
    float d_lv;     // d val / d model log variance
    float d_mean;   // d val / d model mean
};
__device__ __forceinline__ float vb_cdf(float z, float& dcdf) {
    const float k = 0.7978845608028654f;                       // sqrt(2/pi)
    const float th = tanhf(k * (z + 0.044715f * (z * z * z)));
    dcdf = 0.5f * (1.f - th * th) * k * (1.f + 3.f * 0.044715f * z * z);
    return 0.5f * (1.f + th);
}
__device__ __forceinline__ VbElem vb_elem(float x0, float true_mean, float true_lv, float mean, float lv, bool t0) {
    VbElem r;
    if (!t0) {                                                  // normal_kl (tools/losses.py:12-39)
        const float e2 = expf(-lv), d = true_mean - mean, ratio = expf(true_lv - lv);
        r.val = 0.5f * (-1.0f + lv - true_lv + ratio + (d * d) * e2);
        r.d_lv = 0.5f * (1.f - ratio - (d * d) * e2);
        r.d_mean = -d * e2;
        return r;
    }
    // -discretized_gaussian_log_likelihood(x0; mean, 0.5*lv) (tools/losses.py:50-76)
    const float cx = x0 - mean, inv = expf(-(0.5f * lv));
    const float pin = inv * (cx + 1.0f / 255.0f), mnn = inv * (cx - 1.0f / 255.0f);
    float dp, dm;
    const float cp = vb_cdf(pin, dp), cm = vb_cdf(mnn, dm);
    float lp, g_pin = 0.f, g_min = 0.f;                         // d log_prob / d plus_in, / d min_in
    if (x0 < -0.999f) {
        lp = logf(fmaxf(cp, 1e-12f));
        if (cp >= 1e-12f) g_pin = dp / cp;
    } else if (x0 > 0.999f) {
        const float q = 1.f - cm;
        lp = logf(fmaxf(q, 1e-12f));
        if (q >= 1e-12f) g_min = -dm / q;
    } else {
        const float dl = cp - cm;
        lp = logf(fmaxf(dl, 1e-12f));
        if (dl >= 1e-12f) { g_pin = dp / dl; g_min = -dm / dl; }
    }
    r.val = -lp;
    r.d_lv = 0.5f * (g_pin * pin + g_min * mnn);               // d plus_in / d lv = -plus_in / 2
    r.d_mean = inv * (g_pin + g_min);                           // d plus_in / d mean = -inv_stdv
    return r;
}

__global__ void vb_fwd_kernel(const float* __restrict__ mean_out, const float* __restrict__ var_out, const float* __restrict__ x0,
                              const float* __restrict__ xt, const float* __restrict__ coef, int mean_mode, int var_mode,
                              float scale, float* __restrict__ vb, int64_t n) {
    __shared__ float scratch[16];
    const int b = blockIdx.x;
    float c[SS_NCOEF];
#pragma unroll
    for (int i = 0; i < SS_NCOEF; ++i) c[i] = coef[(int64_t)b * SS_NCOEF + i];
    const bool t0 = c[11] != 0.f;
    const int64_t base = (int64_t)b * n;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float x = x0[base + i], z = xt[base + i];
        const Pmv p = p_mean_variance(c, mean_mode, var_mode, 0, mean_out[base + i], var_out ? var_out[base + i] : 0.f, z);
        acc += vb_elem(x, c[2] * x + c[3] * z, c[4], p.mean, p.lv, t0).val;
    }
    const float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) vb[b] = scale * ((tot / (float)n) / 0.6931471805599453f);
}

__global__ void vb_bwd_kernel(const float* __restrict__ mean_out, const float* __restrict__ var_out, const float* __restrict__ x0,
                              const float* __restrict__ xt, const float* __restrict__ coef, int mean_mode, int var_mode,
                              float scale, const float* __restrict__ gvb, float* __restrict__ d_mean, float* __restrict__ d_var,
                              int64_t n) {
    const int b = blockIdx.y;
    float c[SS_NCOEF];
#pragma unroll
    for (int i = 0; i < SS_NCOEF; ++i) c[i] = coef[(int64_t)b * SS_NCOEF + i];
    const bool t0 = c[11] != 0.f;
    const float g = gvb[b] * scale / ((float)n * 0.6931471805599453f);
    const float dlv_dv = var_mode == 2 ? 0.5f * (c[5] - c[4]) : 1.f;
    const float dmean_dm = mean_mode == 1 ? 1.f : c[2] * c[1];
    const int64_t base = (int64_t)b * n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = x0[base + i], z = xt[base + i];
        const Pmv p = p_mean_variance(c, mean_mode, var_mode, 0, mean_out[base + i], var_out ? var_out[base + i] : 0.f, z);
        const VbElem e = vb_elem(x, c[2] * x + c[3] * z, c[4], p.mean, p.lv, t0);
        if (d_var) d_var[base + i] = g * e.d_lv * dlv_dv;
        if (d_mean) d_mean[base + i] = g * e.d_mean * dmean_dm;
    }
}

extern "C" int vaw_vb_fwd(const float* mean_out, const float* var_out, const float* x0, const float* x_t, const float* coef,
                          int mean_mode, int var_mode, float scale, float* vb, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0 && mean_out && x0 && x_t && coef && vb, "vb_fwd: bad arguments");
    VAW_CHECK_ARG((mean_mode == 0 || mean_mode == 1) && var_mode >= 0 && var_mode <= 2 && (var_mode == 0 || var_out),
                  "vb_fwd: bad modes (learned variance needs var_out)");
    vb_fwd_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(mean_out, var_out, x0, x_t, coef, mean_mode, var_mode, scale, vb, per_sample);
    VAW_CHECK_LAUNCH("vb_fwd");
    return VAW_OK;
}

extern "C" int vaw_vb_bwd(const float* mean_out, const float* var_out, const float* x0, const float* x_t, const float* coef,
                          int mean_mode, int var_mode, float scale, const float* gvb, float* d_mean, float* d_var, int B,
                          int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0 && mean_out && x0 && x_t && coef && gvb && (d_mean || d_var), "vb_bwd: bad arguments");
    VAW_CHECK_ARG((mean_mode == 0 || mean_mode == 1) && var_mode >= 0 && var_mode <= 2 && (var_mode == 0 || var_out) &&
                      (var_mode != 0 || !d_var),
                  "vb_bwd: bad modes");
    vb_bwd_kernel<<<row_grid(per_sample, B), 256, 0, (hipStream_t)stream>>>(mean_out, var_out, x0, x_t, coef, mean_mode, var_mode, scale,
                                                                            gvb, d_mean, d_var, per_sample);
    VAW_CHECK_LAUNCH("vb_bwd");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Likelihood evaluation (calc_bpd_loop): the three per-sample scalars of one evaluated timestep in one pass over
// (model mean output, model var values, x0, x_t, noise): 20 B/element read (16 with a fixed variance), nothing of
// [B, per_sample] shape written.
//   pred  = p_mean_variance's, clamped to [-1,1] if clip               (p_mean_variance :343-368)
//   vb    = mean(t==0 ? decoder NLL : KL(q(x_{t-1}|x_t,x0) || p(x_{t-1}|x_t))) / ln 2    (vb_elem, as vb_fwd_kernel)
//   xmse  = mean((pred - x0)^2)                                       (:989)
//   mse   = mean((eps - noise)^2),  eps = (ra*x_t - pred) / rm1       (:990-991, :411-415; not re-associated)
// One workgroup per row; a thread sums its elements in index order (W*i .. W*i + W-1 of each of its items), then wave
// shuffles + one LDS hop (block_sum): a fixed order that depends on per_sample and W only, never on B.  Row b writes
// out[(b % group)*out_ld + b / group]: a launch over K stacked timesteps of `group` samples fills K adjacent columns of the
// [N, T] outputs.  mean_out / var_out rows are model_ld elements apart (the two halves of one [B, 2C, H, W] model output
// are read in place); every other tensor is [B, per_sample] contiguous.
// ---------------------------------------------------------------------------------------------
struct BpdAcc { float vb, xm, ms; };
__device__ __forceinline__ void bpd_elem(const float* c, int mean_mode, int var_mode, int clip, bool t0, float m, float v, float x,
                                         float z, float nz, BpdAcc& a) {
    const Pmv p = p_mean_variance(c, mean_mode, var_mode, clip, m, v, z);
    a.vb += vb_elem(x, c[2] * x + c[3] * z, c[4], p.mean, p.lv, t0).val;
    const float dx = p.pred - x;
    a.xm += dx * dx;
    const float de = (c[6] * z - p.pred) / c[7] - nz;
    a.ms += de * de;
}

template <int W>
__global__ void __launch_bounds__(1024)
bpd_terms_kernel(const float* __restrict__ mean_out, const float* __restrict__ var_out, int64_t model_ld,
                 const float* __restrict__ x0, const float* __restrict__ xt, const float* __restrict__ noise,
                 const float* __restrict__ coef, int mean_mode, int var_mode, int clip, float* __restrict__ vb,
                 float* __restrict__ xmse, float* __restrict__ mse, int64_t out_ld, int group, int64_t n) {
    __shared__ float scratch[16];
    const int b = blockIdx.x;
    float c[SS_NCOEF];
#pragma unroll
    for (int i = 0; i < 12; ++i) c[i] = coef[b * SS_NCOEF + i];
    const bool t0 = c[11] != 0.f;
    const float* mr = mean_out + (int64_t)b * model_ld;
    const float* vr = var_out ? var_out + (int64_t)b * model_ld : nullptr;
    const float* xr = x0 + (int64_t)b * n;
    const float* zr = xt + (int64_t)b * n;
    const float* nr = noise + (int64_t)b * n;
    BpdAcc a = {0.f, 0.f, 0.f};
    for (int64_t i = threadIdx.x; i < n / W; i += blockDim.x) {
        float m[W], x[W], z[W], e[W], v[W] = {};
        loadw<W>(mr + W * i, m);
        loadw<W>(xr + W * i, x);
        loadw<W>(zr + W * i, z);
        loadw<W>(nr + W * i, e);
        if (vr) loadw<W>(vr + W * i, v);
#pragma unroll
        for (int j = 0; j < W; ++j) bpd_elem(c, mean_mode, var_mode, clip, t0, m[j], v[j], x[j], z[j], e[j], a);
    }
    const float tv = block_sum(a.vb, scratch), tx = block_sum(a.xm, scratch), tm = block_sum(a.ms, scratch);
    if (threadIdx.x == 0) {
        const int64_t o = (int64_t)(b % group) * out_ld + b / group;
        vb[o] = (tv / (float)n) / 0.6931471805599453f;
        xmse[o] = tx / (float)n;
        mse[o] = tm / (float)n;
    }
}

extern "C" int vaw_bpd_terms(const float* mean_out, const float* var_out, int64_t model_ld, const float* x0, const float* x_t,
                             const float* noise, const float* coef, int mean_mode, int var_mode, int clip_denoised, float* vb,
                             float* xstart_mse, float* mse, int64_t out_ld, int group, int B, int64_t per_sample,
                             vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "bpd_terms: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(mean_out && x0 && x_t && noise && coef && vb && xstart_mse && mse, "bpd_terms: null pointer");
    VAW_CHECK_ARG(model_ld >= per_sample, "bpd_terms: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG((mean_mode == 0 || mean_mode == 1) && var_mode >= 0 && var_mode <= 2 && (var_mode == 0 || var_out),
                  "bpd_terms: bad modes (mean_mode %d, var_mode %d; learned variance needs var_out)", mean_mode, var_mode);
    VAW_CHECK_ARG(group > 0 && B % group == 0 && out_ld >= B / group, "bpd_terms: bad output layout (group %d, out_ld %ld, B %d)",
                  group, (long)out_ld, B);
    VAW_LAUNCH_W(bpd_terms_kernel, vec4_ok(per_sample, model_ld, {mean_out, var_out, x0, x_t, noise}), B, 1024, stream, mean_out, var_out,
                 model_ld, x0, x_t, noise, coef, mean_mode, var_mode, clip_denoised, vb, xstart_mse, mse, out_ld, group, per_sample);
    VAW_CHECK_LAUNCH("bpd_terms");
    return VAW_OK;
}

// _prior_bpd :932-948: KL(q(x_T | x_0) || N(0, I)) / ln 2 per sample; q_mean_variance :217-232 at t = T-1 gives
// mean = sqrt_abar * x0 and log variance = log_1m_abar, normal_kl (tools/losses.py:33-39) against mean 0, log variance 0.
__global__ void __launch_bounds__(1024)
prior_bpd_kernel(const float* __restrict__ x0, float sqrt_abar, float log_1m_abar, float* __restrict__ out, int64_t n, int vec) {
    __shared__ float scratch[16];
    const int b = blockIdx.x;
    const float* xr = x0 + (int64_t)b * n;
    const float k = -1.0f + 0.f - log_1m_abar + expf(log_1m_abar - 0.f);
    float acc = 0.f;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
        const f32x4 m = sqrt_abar * load4(xr + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += 0.5f * (k + (m[j] * m[j]) * 1.f);
    }
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
        const float m = sqrt_abar * xr[i];
        acc += 0.5f * (k + (m * m) * 1.f);
    }
    const float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) out[b] = (tot / (float)n) / 0.6931471805599453f;
}

extern "C" int vaw_prior_bpd(const float* x0, float sqrt_abar_last, float log_one_minus_abar_last, float* prior_bpd, int B,
                             int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "prior_bpd: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(x0 && prior_bpd, "prior_bpd: null pointer");
    prior_bpd_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(x0, sqrt_abar_last, log_one_minus_abar_last, prior_bpd, per_sample,
                                                          per_sample % 4 == 0 && al16(x0));
    VAW_CHECK_LAUNCH("prior_bpd");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// One reverse-process step (sampling side): classifier-free guidance + p_mean_variance + the sampler's update, fused.
//   kind 0: no sample (p_mean_variance only)
//        1: ancestral p_sample:  sample = mean + (t != 0) * exp(lv/2) * noise
//        2: ddim_sample:         eps = (ra*x - pred)/rm1, sigma = (eta*s1)*s2,
//                                sample = pred*sqrt_abp + sqrt(1 - abp - sigma^2)*eps + (t != 0) * sigma * noise
//        3: ddim_reverse_sample (:653-689, eta = 0, the DDIM ODE run towards noise): sample = pred*sqrt(abn) + sqrt(1 - abn)*eps;
//           no noise, and the model variance does not enter
// The model output of the stacked [2N, ...] guided call is read in place: row b of each of the four quarters (conditional /
// unconditional half of the batch, mean / variance channels) starts model_ld floats after row b-1.  mu == NULL: no guidance,
// the plain step over split halves.  Everything else is [B, n] contiguous; outputs may be NULL.  One grid row per sample.
// ---------------------------------------------------------------------------------------------
// what a launch derives from one coefficient row before its element loop
struct SsRow { float c[SS_NCOEF]; float mask, sigma, ddim_c, rev_a, rev_b; };
__device__ __forceinline__ void ss_row(const float* __restrict__ coef, int b, float eta, SsRow& r) {
#pragma unroll
    for (int i = 0; i < SS_NCOEF; ++i) r.c[i] = coef[(int64_t)b * SS_NCOEF + i];
    r.mask = r.c[11] != 0.f ? 0.f : 1.f;
    r.sigma = (eta * r.c[9]) * r.c[12];
    r.ddim_c = sqrtf(1.f - r.c[10] - r.sigma * r.sigma);
    r.rev_a = sqrtf(r.c[13]);
    r.rev_b = sqrtf(1.f - r.c[13]);
}
struct SsOut { float sample, pred, mean, lv; };
// nz: the noise of the element (read by kinds 1 and 2 only)
__device__ __forceinline__ SsOut ss_elem(const SsRow& r, int kind, int mean_mode, int var_mode, int clip, float m, float v,
                                         float xv, float nz) {
    const float* c = r.c;
    const Pmv p = p_mean_variance(c, mean_mode, var_mode, clip, m, v, xv);
    SsOut o = {0.f, p.pred, p.mean, p.lv};
    if (kind == 1) {
        o.sample = p.mean + (r.mask * expf(0.5f * p.lv)) * nz;
    } else if (kind >= 2) {
        const float eps = (c[6] * xv - p.pred) / c[7];
        if (kind == 2) {
            const float mp = p.pred * c[8] + r.ddim_c * eps;
            o.sample = mp + (r.mask * r.sigma) * nz;
        } else {
            o.sample = p.pred * r.rev_a + r.rev_b * eps;
        }
    }
    return o;
}

template <int W>
__global__ void guided_sample_step_kernel(const float* __restrict__ mc, const float* __restrict__ mu, const float* __restrict__ vc,
                                          const float* __restrict__ vu, int64_t model_ld, float gs, const float* __restrict__ x,
                                          const float* __restrict__ noise, const float* __restrict__ coef, int kind,
                                          int mean_mode, int var_mode, int clip, float eta, float* __restrict__ sample,
                                          float* __restrict__ pred_out, float* __restrict__ mean_o,
                                          float* __restrict__ logvar_o, int64_t n) {
    const int b = blockIdx.y;
    SsRow r;
    ss_row(coef, b, eta, r);
    const int64_t base = (int64_t)b * n, mbase = (int64_t)b * model_ld;
    const bool guided = mu != nullptr, var = var_mode != 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i, mo = mbase + W * i;
        float m[W], v[W] = {}, xv[W], nz[W] = {};
        loadw<W>(mc + mo, m);
        if (var) loadw<W>(vc + mo, v);
        loadw<W>(x + o, xv);
        if (noise) loadw<W>(noise + o, nz);
        if (guided) {
            float m0[W], v0[W] = {};
            loadw<W>(mu + mo, m0);
            if (var) loadw<W>(vu + mo, v0);
#pragma unroll
            for (int j = 0; j < W; ++j) { m[j] = cfg_mix(m[j], m0[j], gs); if (var) v[j] = cfg_mix(v[j], v0[j], gs); }
        }
        float s[W], p[W], mn[W], lv[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const SsOut e = ss_elem(r, kind, mean_mode, var_mode, clip, m[j], v[j], xv[j], nz[j]);
            s[j] = e.sample; p[j] = e.pred; mn[j] = e.mean; lv[j] = e.lv;
        }
        if (pred_out) storew<W>(pred_out + o, p);
        if (mean_o) storew<W>(mean_o + o, mn);
        if (logvar_o) storew<W>(logvar_o + o, lv);
        if (kind) storew<W>(sample + o, s);
    }
}

extern "C" int vaw_guided_sample_step(int kind, const float* mean_cond, const float* mean_uncond, const float* var_cond,
                                      const float* var_uncond, int64_t model_ld, float guidance_scale, const float* x,
                                      const float* noise, const float* coef, int mean_mode, int var_mode, int clip_denoised,
                                      float eta, float* sample, float* pred_xstart, float* mean, float* log_variance, int B,
                                      int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "guided_sample_step: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(mean_cond && x && coef && kind >= 0 && kind <= 3, "guided_sample_step: null pointer or bad kind %d", kind);
    VAW_CHECK_ARG(model_ld >= per_sample, "guided_sample_step: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG(kind != 3 || (!noise && !var_cond && !var_uncond && var_mode == 0 && !mean && !log_variance),
                  "guided_sample_step: kind 3 takes no noise and no variance (var_mode 0) and writes sample and pred_xstart only");
    VAW_CHECK_ARG((mean_mode == 0 || mean_mode == 1) && var_mode >= 0 && var_mode <= 2 && (var_mode == 0 || var_cond) &&
                      (var_mode == 0 || !mean_uncond || var_uncond),
                  "guided_sample_step: bad modes (learned variance needs var_cond, and var_uncond when guided)");
    VAW_CHECK_ARG(kind == 0 || (sample && (noise || kind == 3)), "guided_sample_step: kind 1/2 need noise and sample, kind 3 sample (null pointer)");
    if (kind == 0) noise = nullptr;
    if (var_mode == 0) var_cond = var_uncond = nullptr;
    if (!mean_uncond) var_uncond = nullptr;
    const bool vec = vec4_ok(per_sample, model_ld, {mean_cond, mean_uncond, var_cond, var_uncond, x, noise, sample, pred_xstart, mean,
                                                    log_variance});
    VAW_LAUNCH_W(guided_sample_step_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, mean_cond, mean_uncond,
                 var_cond, var_uncond, model_ld, guidance_scale, x, noise, coef, kind, mean_mode, var_mode, clip_denoised, eta, sample,
                 pred_xstart, mean, log_variance, per_sample);
    VAW_CHECK_LAUNCH("guided_sample_step");
    return VAW_OK;
}

template <int W>
__global__ void cfg_combine_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, int64_t model_ld, float gs,
                                   float* __restrict__ out, int64_t n) {
    const int64_t base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * model_ld;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        float c[W], u[W];
        loadw<W>(cond + mbase + W * i, c);
        loadw<W>(uncond + mbase + W * i, u);
#pragma unroll
        for (int j = 0; j < W; ++j) c[j] = cfg_mix(c[j], u[j], gs);
        storew<W>(out + base + W * i, c);
    }
}

extern "C" int vaw_cfg_combine(const float* cond, const float* uncond, int64_t model_ld, float guidance_scale, float* out, int B,
                               int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "cfg_combine: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(cond && uncond && out, "cfg_combine: null pointer");
    VAW_CHECK_ARG(model_ld >= per_sample, "cfg_combine: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    const bool vec = vec4_ok(per_sample, model_ld, {cond, uncond, out});
    VAW_LAUNCH_W(cfg_combine_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, cond, uncond, model_ld,
                 guidance_scale, out, per_sample);
    VAW_CHECK_LAUNCH("cfg_combine");
    return VAW_OK;
}

// [B, C, H, W] samples in [-1, 1] -> [B, H, W, C] bytes:  v = (x + 1) * 127.5 in the source precision (sum and product each
// rounded), clamped to [0, 255], truncated toward zero.  fmax(NaN, 0) is 0, so NaN writes 0.
__device__ __forceinline__ unsigned quant_u8(float x) { return (unsigned)(int)fminf(fmaxf((x + 1.f) * 127.5f, 0.f), 255.f); }
__device__ __forceinline__ unsigned quant_u8(double x) { return (unsigned)(int)fmin(fmax((x + 1.0) * 127.5, 0.0), 255.0); }

// Aligned form (HW % 4 == 0, src 16-byte and dst 4-byte aligned, C <= 4): a thread takes 4 neighbouring pixels of one image,
// reads 16 (f32) or 32 (f64) contiguous bytes of each channel plane -- a wave reads 1 or 2 KiB of a plane per instruction --
// and writes their 4*C interleaved bytes as C whole words; the lanes of a wave write one contiguous run.
template <typename T, int C>
__global__ void finish_images_vec_kernel(const T* __restrict__ src, uint32_t* __restrict__ dst, int64_t B, int64_t HW) {
    const int64_t groups = HW / 4, total = B * groups;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = idx / groups, g = idx - b * groups;
        uint32_t w[C];
#pragma unroll
        for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            T v[4];
            loadw<4>(src + (b * C + c) * HW + 4 * g, v);
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int j = px * C + c;
                w[j >> 2] |= quant_u8(v[px]) << (8 * (j & 3));
            }
        }
        uint32_t* o = dst + idx * C;          // (b*HW + 4g) * C bytes = idx * C words
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = w[k];
    }
}

// General form (any C, H, W, any alignment): a thread owns one 4-byte-aligned word of the destination.  A word that lies
// wholly inside [dst, dst + total) is stored whole; the ragged first and last words are stored byte by byte, so nothing
// outside the destination is written.  a0 = dst & 3; dst_al = dst - a0.
template <typename T>
__global__ void finish_images_gen_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst_al, int a0, int64_t total, int64_t C,
                                         int64_t HW) {
    const int64_t words = (a0 + total + 3) / 4;
    for (int64_t wi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; wi < words; wi += (int64_t)gridDim.x * blockDim.x) {
        uint32_t w = 0u;
        bool whole = true;
        uint8_t q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t k = 4 * wi + j - a0;          // flat index into [B, H, W, C]
            q[j] = 0;
            if (k < 0 || k >= total) { whole = false; continue; }
            const int64_t pix = k / C, c = k - pix * C, b = pix / HW, p = pix - b * HW;
            q[j] = (uint8_t)quant_u8(src[(b * C + c) * HW + p]);
            w |= (uint32_t)q[j] << (8 * j);
        }
        if (whole) {
            *reinterpret_cast<uint32_t*>(dst_al + 4 * wi) = w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = 4 * wi + j - a0;
                if (k >= 0 && k < total) dst_al[4 * wi + j] = q[j];
            }
        }
    }
}

template <typename T>
static int finish_images_launch(const T* src, uint8_t* dst, int64_t B, int64_t C, int64_t HW, hipStream_t st) {
    const int64_t total = B * C * HW;
    const bool vec = HW % 4 == 0 && C <= 4 && al16(src) && ((uintptr_t)dst & 3) == 0;
    if (vec) {
        const int grid = stream_grid(B * (HW / 4), 256);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        switch ((int)C) {
            case 1: finish_images_vec_kernel<T, 1><<<grid, 256, 0, st>>>(src, d, B, HW); break;
            case 2: finish_images_vec_kernel<T, 2><<<grid, 256, 0, st>>>(src, d, B, HW); break;
            case 3: finish_images_vec_kernel<T, 3><<<grid, 256, 0, st>>>(src, d, B, HW); break;
            default: finish_images_vec_kernel<T, 4><<<grid, 256, 0, st>>>(src, d, B, HW); break;
        }
    } else {
        const int a0 = (int)((uintptr_t)dst & 3);
        const int grid = stream_grid((a0 + total + 3) / 4, 256);
        finish_images_gen_kernel<T><<<grid, 256, 0, st>>>(src, dst - a0, a0, total, C, HW);
    }
    return 0;
}

extern "C" int vaw_finish_images(const void* src, int src_f64, uint8_t* dst, int B, int C, int H, int W, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "finish_images: bad sizes B=%d C=%d H=%d W=%d", B, C, H, W);
    VAW_CHECK_ARG(src && dst, "finish_images: null pointer");
    VAW_CHECK_ARG(src_f64 == 0 || src_f64 == 1, "finish_images: src_f64 must be 0 (f32) or 1 (f64), got %d", src_f64);
    VAW_CHECK_ARG(((uintptr_t)src & (src_f64 ? 7 : 3)) == 0, "finish_images: source not aligned to its element size");
    const int64_t HW = (int64_t)H * W;
    if (src_f64) finish_images_launch(static_cast<const double*>(src), dst, B, C, HW, (hipStream_t)stream);
    else finish_images_launch(static_cast<const float*>(src), dst, B, C, HW, (hipStream_t)stream);
    VAW_CHECK_LAUNCH("finish_images");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Small conditioning-path kernels ([B, D]-sized)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void timestep_embedding_kernel(const float* __restrict__ t, T* __restrict__ out, int B, int dim,
                                          float neg_log_period) {
    const int half = dim / 2;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < (int64_t)B * dim;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx / dim), j = (int)(idx % dim);
        float v = 0.f;
        if (j < 2 * half) {
            const int i = j < half ? j : j - half;
            // same op order as the reference: exp(-ln(P) * i / half) in f32, then t * f
            const float f = expf(neg_log_period * (float)i / (float)half);
            const float ang = t[b] * f;
            v = j < half ? cosf(ang) : sinf(ang);
        }
        out[idx] = from_f32<T>(v);
    }
}

extern "C" int vaw_timestep_embedding(vaw_dtype dt, const float* t, void* out, int B, int dim, float max_period,
                                      vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && dim > 0, "timestep_embedding: bad sizes");
    const float nl = -logf(max_period);
    int grid = stream_grid((int64_t)B * dim, 256);
    if (dt == VAW_F32)
        timestep_embedding_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(t, (float*)out, B, dim, nl);
    else
        timestep_embedding_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(t, (bf16_t*)out, B, dim, nl);
    VAW_CHECK_LAUNCH("timestep_embedding");
    return VAW_OK;
}

template <typename T>
__global__ void silu_fwd_kernel(const float* __restrict__ x, T* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = from_f32<T>(silu_f(x[i]));
}
__global__ void silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dx[i] = dy[i] * silu_grad_f(x[i]);
}
// the same pass, leaving the bf16 rounding of dx beside it: the operand of the weight-gradient GEMM that follows (what
// cast_bf16_kernel makes of dx in a launch of its own)
__global__ void silu_bwd_cast_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                     bf16_t* __restrict__ dx_act, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = dy[i] * silu_grad_f(x[i]);
        dx[i] = v;
        dx_act[i] = (bf16_t)v;
    }
}
extern "C" int vaw_silu_fwd(vaw_dtype dt, const float* x, void* out, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "silu_fwd: n<=0");
    int grid = stream_grid(n, 256);
    if (dt == VAW_F32) silu_fwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(x, (float*)out, n);
    else silu_fwd_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(x, (bf16_t*)out, n);
    VAW_CHECK_LAUNCH("silu_fwd");
    return VAW_OK;
}
extern "C" int vaw_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "silu_bwd: n<=0");
    silu_bwd_kernel<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, dy, dx, n);
    VAW_CHECK_LAUNCH("silu_bwd");
    return VAW_OK;
}

__global__ void add_embedding_kernel(const float* __restrict__ a, const float* __restrict__ table,
                                     const int64_t* __restrict__ idx, float* __restrict__ out, int B, int D, int rows) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (int64_t)B * D; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / D), d = (int)(i % D);
        const int64_t r = idx[b];
        out[i] = a[i] + ((r >= 0 && r < rows) ? table[r * D + d] : __builtin_nanf(""));
    }
}
// dtable[r,:] = beta*dtable[r,:] + sum over {b : idx[b]==r} dc[b,:], b ascending.  One workgroup per table row: the index vector
// is compared with r 1024 entries at a time, one entry per thread and round, and every wave leaves the 64-bit mask of its matches
// in LDS; a thread owns columns t, t + 256, ... and adds the matching rows by walking the set bits of those masks in batch order.
// Deterministic, no pre-zeroing pass over the table.  (Round 3 had one thread per table ELEMENT scanning the whole index vector
// from global memory: 53 us for a 1001 x 768 table at batch 256.  Round 4 staged the indices in LDS and let every thread test all
// of them one after the other, a dependent LDS read and a branch per entry: 24 us, nearly all of it in rows nobody indexed.  With
// the compare done once per entry a row without matches costs one round.)
__global__ void __launch_bounds__(256)
embedding_bwd_kernel(const float* __restrict__ dc, const int64_t* __restrict__ idx, float* __restrict__ dtable, int B, int D,
                     int rows, float beta) {
    __shared__ unsigned long long s_mask[16];                 // matches of entries b0 + 64 w .. b0 + 64 w + 63
    const int r = blockIdx.x;
    constexpr int MAXC = 8;                                   // columns per thread held in registers (D <= 2048); wider tables loop
    for (int d0 = 0; d0 < D; d0 += 256 * MAXC) {
        float acc[MAXC];
#pragma unroll
        for (int j = 0; j < MAXC; ++j) acc[j] = 0.f;
        for (int b0 = 0; b0 < B; b0 += 1024) {
            const int nb = B - b0 < 1024 ? B - b0 : 1024;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = threadIdx.x + 256 * k;          // wave w of round k covers entries 64 (4 k + w) ..
                const unsigned long long m = __ballot(i < nb && idx[b0 + (i < nb ? i : 0)] == (int64_t)r);
                if ((threadIdx.x & 63) == 0) s_mask[4 * k + (threadIdx.x >> 6)] = m;
            }
            __syncthreads();
            for (int w = 0; w < 16; ++w) {
                unsigned long long m = s_mask[w];             // uniform: every thread walks the same bits
                while (m) {
                    const int i = 64 * w + __builtin_ctzll(m);
                    m &= m - 1;
                    const float* src = dc + (int64_t)(b0 + i) * D + d0;
#pragma unroll
                    for (int j = 0; j < MAXC; ++j) {
                        const int d = threadIdx.x + 256 * j;
                        if (d0 + d < D) acc[j] += src[d];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int d = d0 + threadIdx.x + 256 * j;
            if (d < D) {
                float* o = dtable + (int64_t)r * D + d;
                *o = (beta != 0.f ? beta * *o : 0.f) + acc[j];
            }
        }
    }
}
extern "C" int vaw_silu_bwd_cast(const float* x, const float* dy, float* dx, void* dx_bf16, int64_t n, vaw_stream stream) {
    if (!dx_bf16) return vaw_silu_bwd(x, dy, dx, n, stream);
    VAW_CHECK_ARG(n > 0, "silu_bwd_cast: n<=0");
    silu_bwd_cast_kernel<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, dy, dx, (bf16_t*)dx_bf16, n);
    VAW_CHECK_LAUNCH("silu_bwd_cast");
    return VAW_OK;
}

extern "C" int vaw_add_embedding(const float* a, const float* table, const int64_t* idx, float* out, int B, int D,
                                 int num_rows, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && D > 0 && num_rows > 0, "add_embedding: bad sizes");
    add_embedding_kernel<<<stream_grid((int64_t)B * D, 256), 256, 0, (hipStream_t)stream>>>(a, table, idx, out, B, D, num_rows);
    VAW_CHECK_LAUNCH("add_embedding");
    return VAW_OK;
}
extern "C" int vaw_embedding_bwd(const float* dc, const int64_t* idx, float* dtable, int B, int D, int num_rows,
                                 float beta, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && D > 0 && num_rows > 0, "embedding_bwd: bad sizes");
    embedding_bwd_kernel<<<num_rows, 256, 0, (hipStream_t)stream>>>(dc, idx, dtable, B, D, num_rows, beta);
    VAW_CHECK_LAUNCH("embedding_bwd");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// patchify / unpatchify: index shuffles between NCHW images and token rows.
//   patch-embed token column  k = (c*p + i)*p + j      (Conv2d weight [D, C, p, p] flattened)
//   final-layer token column  k = (i*p + j)*C + c      (einsum nhwpqc->nchpwq, dit.py:253-255)
// One thread per image element; the image side is always the coalesced one.
// ---------------------------------------------------------------------------------------------
template <typename T, bool CONV_ORDER, bool TO_TOKENS>
__global__ void patch_shuffle_kernel(const float* __restrict__ img_in, float* __restrict__ img_out,
                                     const float* __restrict__ tok_in_f32, T* __restrict__ tok_out, int B, int C, int H,
                                     int W, int p) {
    const int hp = H / p, wp = W / p;
    const int64_t total = (int64_t)B * C * H * W;
    const int K = C * p * p;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int x = (int)(e % W);
        int64_t r = e / W;
        int y = (int)(r % H);
        r /= H;
        int c = (int)(r % C);
        int b = (int)(r / C);
        const int ty = y / p, i = y % p, tx = x / p, j = x % p;
        const int64_t row = ((int64_t)b * hp + ty) * wp + tx;
        const int col = CONV_ORDER ? (c * p + i) * p + j : (i * p + j) * C + c;
        if (TO_TOKENS) tok_out[row * K + col] = from_f32<T>(img_in[e]);
        else img_out[e] = tok_in_f32[row * K + col];
    }
}

extern "C" int vaw_patchify(vaw_dtype dt, const float* img, void* tok, int B, int C, int H, int W, int p,
                            vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0, "patchify: bad sizes");
    int grid = stream_grid((int64_t)B * C * H * W, 256);
    if (dt == VAW_F32)
        patch_shuffle_kernel<float, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(img, nullptr, nullptr, (float*)tok, B, C, H, W, p);
    else
        patch_shuffle_kernel<bf16_t, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(img, nullptr, nullptr, (bf16_t*)tok, B, C, H, W, p);
    VAW_CHECK_LAUNCH("patchify");
    return VAW_OK;
}
extern "C" int vaw_patchify_bwd(const float* dtok, float* dimg, int B, int C, int H, int W, int p, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0, "patchify_bwd: bad sizes");
    int grid = stream_grid((int64_t)B * C * H * W, 256);
    patch_shuffle_kernel<float, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(nullptr, dimg, dtok, nullptr, B, C, H, W, p);
    VAW_CHECK_LAUNCH("patchify_bwd");
    return VAW_OK;
}
extern "C" int vaw_unpatchify(vaw_dtype dt, const float* tok, float* img, int B, int C, int H, int W, int p,
                              vaw_stream stream) {
    (void)dt;
    VAW_CHECK_ARG(B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0, "unpatchify: bad sizes");
    int grid = stream_grid((int64_t)B * C * H * W, 256);
    patch_shuffle_kernel<float, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(nullptr, img, tok, nullptr, B, C, H, W, p);
    VAW_CHECK_LAUNCH("unpatchify");
    return VAW_OK;
}
extern "C" int vaw_unpatchify_bwd(vaw_dtype dt, const float* dimg, void* dtok, int B, int C, int H, int W, int p,
                                  vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0, "unpatchify_bwd: bad sizes");
    int grid = stream_grid((int64_t)B * C * H * W, 256);
    if (dt == VAW_F32)
        patch_shuffle_kernel<float, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(dimg, nullptr, nullptr, (float*)dtok, B, C, H, W, p);
    else
        patch_shuffle_kernel<bf16_t, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(dimg, nullptr, nullptr, (bf16_t*)dtok, B, C, H, W, p);
    VAW_CHECK_LAUNCH("unpatchify_bwd");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Optimizer: sum of squares, fused AdamW + EMA + bf16 shadow, EMA alone, cast.
// 36 B/param algorithmic traffic for the fused pass (p,g,m,v,ema read; p,m,v,ema written) + 2 B shadow.
// ---------------------------------------------------------------------------------------------
#define SUMSQ_MAX_BLOCKS 2048
__global__ void sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float scratch[16];
    float acc = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = load4(g + 4 * i);
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        acc += g[i] * g[i];
    float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ void sumsq_final_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out, int accumulate) {
    __shared__ float scratch[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) acc += partial[i];
    float tot = block_sum(acc, scratch);
    if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + tot;
}
extern "C" int64_t vaw_sumsq_workspace_floats(void) { return SUMSQ_MAX_BLOCKS; }
extern "C" int vaw_sumsq(const float* g, int64_t n, float* sumsq_out, int accumulate, float* workspace,
                         vaw_stream stream) {
    VAW_CHECK_ARG(n > 0 && ((uintptr_t)g & 15) == 0 && workspace, "sumsq: n<=0, unaligned or no workspace");
    const int grid = stream_grid(n / 4 + 1, 256);
    sumsq_partial_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(g, n, workspace);
    sumsq_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(workspace, grid, sumsq_out, accumulate);
    VAW_CHECK_LAUNCH("sumsq");
    return VAW_OK;
}

struct AdamArgs {
    float lr, b1, b2, eps, wd, bc1, bc2_sqrt, ema_decay, clip;
    int zero_grad;
};

__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, float& e, bool has_ema, float gs,
                                         const AdamArgs& a) {
    const float gg = g * gs;
    p = p * (1.f - a.lr * a.wd);
    m = m + (gg - m) * (1.f - a.b1);
    v = v * a.b2 + (1.f - a.b2) * gg * gg;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - (a.lr / a.bc1) * (m / denom);
    if (has_ema) e = e * a.ema_decay + p * (1.f - a.ema_decay);
}

// Each workgroup walks contiguous tiles of ADAM_U x 256 float4 per stream (16 KiB of p, g, m, v and ema each): every lane has
// ADAM_U independent 16-byte loads of all five streams in flight before the first use (20 loads per lane instead of 5), a stream's
// accesses stay inside one DRAM page run per tile instead of hopping 8 MiB between iterations, and every byte is touched once per
// step (38 B per parameter, 5 GB for DiT-B: nothing of it is in a cache when the next step comes round) -> non-temporal loads and
// stores.  Round 3's one-float4-per-iteration grid-stride loop ran at 5.0 TB/s of these bytes.
#define ADAM_U 4
__device__ __forceinline__ f32x4 nt_load4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
// GUARDED (vaw_adamw_ema_step_guarded; guard.hip: vaw_step_guard writes the verdict): ok[0] is one word every lane of every workgroup
// reads, so the branch is uniform across the grid.  ok[0] != 0: the pass below, bit for bit.  ok[0] == 0: the step is refused --
// nothing is read and nothing written but the zero_grad store of g, so the masters, the moments, the EMA and the shadow keep the
// last good step's bits.  One text, two instantiations; the unguarded one never looks at `ok`.
template <bool GUARDED>
__global__ void __launch_bounds__(256)
adamw_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                 float* __restrict__ ema, bf16_t* __restrict__ shadow, int64_t n, const float* __restrict__ sumsq, AdamArgs a,
                 const float* __restrict__ hyper, const int32_t* __restrict__ ok) {
    if (GUARDED && ok[0] == 0) {
        if (a.zero_grad) {
            const int64_t n4 = n / 4;
            for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
                store4(g + 4 * i, f32x4{0, 0, 0, 0});
            for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
                g[i] = 0.f;
        }
        return;
    }
    if (hyper) {          // step-dependent scalars from device memory: the launch can then sit in a replayed hipGraph
        a.lr = hyper[0];
        a.bc1 = hyper[1];
        a.bc2_sqrt = sqrtf(hyper[2]);
    }
    float gs = 1.f;
    if (a.clip > 0.f) {
        const float coef = a.clip / (sqrtf(*sumsq) + 1e-6f);
        gs = coef < 1.f ? coef : 1.f;
    }
    const int64_t n4 = n / 4;
    const bool has_ema = ema != nullptr;
    constexpr int64_t TILE = (int64_t)ADAM_U * 256;                  // float4 per tile
    const int64_t n_tiles = n4 / TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t i0 = t * TILE + threadIdx.x;
        f32x4 pv[ADAM_U], gv[ADAM_U], mv[ADAM_U], vv[ADAM_U], ev[ADAM_U];
#pragma unroll
        for (int u = 0; u < ADAM_U; ++u) {
            const int64_t i = 4 * (i0 + 256 * u);
            pv[u] = nt_load4(p + i); gv[u] = nt_load4(g + i); mv[u] = nt_load4(m + i); vv[u] = nt_load4(v + i);
            ev[u] = has_ema ? nt_load4(ema + i) : f32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < ADAM_U; ++u) {
            const int64_t i = 4 * (i0 + 256 * u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pv[u][j], gj = gv[u][j], mj = mv[u][j], vj = vv[u][j], ej = ev[u][j];
                adam_one(pj, gj, mj, vj, ej, has_ema, gs, a);
                pv[u][j] = pj; mv[u][j] = mj; vv[u][j] = vj; ev[u][j] = ej;
            }
            __builtin_nontemporal_store(pv[u], reinterpret_cast<f32x4*>(p + i));
            __builtin_nontemporal_store(mv[u], reinterpret_cast<f32x4*>(m + i));
            __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4*>(v + i));
            if (has_ema) __builtin_nontemporal_store(ev[u], reinterpret_cast<f32x4*>(ema + i));
            if (shadow) store4(shadow + i, pv[u]);          // default policy: the next forward reads the shadow weights first
            if (a.zero_grad) store4(g + i, f32x4{0, 0, 0, 0});
        }
    }
    // the last, partial tile (and n % 4 elements), one element group per thread
    for (int64_t i = n_tiles * TILE + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = load4(p + 4 * i), gv = load4(g + 4 * i), mv = load4(m + 4 * i), vv = load4(v + 4 * i);
        f32x4 ev = has_ema ? load4(ema + 4 * i) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], gj = gv[j], mj = mv[j], vj = vv[j], ej = ev[j];
            adam_one(pj, gj, mj, vj, ej, has_ema, gs, a);
            pv[j] = pj; mv[j] = mj; vv[j] = vj; ev[j] = ej;
        }
        store4(p + 4 * i, pv);
        store4(m + 4 * i, mv);
        store4(v + 4 * i, vv);
        if (has_ema) store4(ema + 4 * i, ev);
        if (shadow) store4(shadow + 4 * i, pv);
        if (a.zero_grad) store4(g + 4 * i, f32x4{0, 0, 0, 0});
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pv = p[i], gv = g[i], mv = m[i], vv = v[i], ev = has_ema ? ema[i] : 0.f;
        adam_one(pv, gv, mv, vv, ev, has_ema, gs, a);
        p[i] = pv; m[i] = mv; v[i] = vv;
        if (has_ema) ema[i] = ev;
        if (shadow) shadow[i] = (bf16_t)pv;
        if (a.zero_grad) g[i] = 0.f;
    }
}
static inline int adam_grid(int64_t n) {
    const int64_t tiles = n / 4 / (ADAM_U * 256);
    const int64_t cap = 256 * 8;
    return (int)(tiles < 1 ? 1 : (tiles > cap ? cap : tiles));
}

// One host side for the four entry points: hyper == nullptr takes the step-dependent scalars from `a`, `guarded` picks the
// instantiation (and then insists on a verdict to read).
static int adamw_launch(const char* what, float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                        const float* hyper, const AdamArgs& a, const float* sumsq, const int32_t* ok, bool guarded, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "%s: n<=0", what);
    VAW_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0 &&
                      ((uintptr_t)shadow_bf16 & 7) == 0, "%s: buffers must be 16-byte aligned", what);
    VAW_CHECK_ARG(a.clip <= 0.f || sumsq != nullptr, "%s: clip needs sumsq", what);
    VAW_CHECK_ARG(!guarded || (ok != nullptr && ((uintptr_t)ok & 3) == 0), "%s: ok must be a 4-byte aligned device int32", what);
    if (guarded)
        adamw_ema_kernel<true><<<adam_grid(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, (bf16_t*)shadow_bf16, n, sumsq, a, hyper, ok);
    else
        adamw_ema_kernel<false><<<adam_grid(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, (bf16_t*)shadow_bf16, n, sumsq, a, hyper, nullptr);
    VAW_CHECK_LAUNCH(what);
    return VAW_OK;
}

extern "C" int vaw_adamw_ema_step(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                  float bc2, float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad,
                                  vaw_stream stream) {
    AdamArgs a{lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), ema_decay, clip_max_norm, zero_grad};
    return adamw_launch("adamw_ema", p, g, m, v, ema, shadow_bf16, n, nullptr, a, sumsq, nullptr, false, stream);
}

extern "C" int vaw_adamw_ema_step_dev(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                                      const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                                      float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad,
                                      vaw_stream stream) {
    VAW_CHECK_ARG(hyper, "adamw_ema_dev: no hyper buffer");
    AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, ema_decay, clip_max_norm, zero_grad};
    return adamw_launch("adamw_ema_dev", p, g, m, v, ema, shadow_bf16, n, hyper, a, sumsq, nullptr, false, stream);
}

extern "C" int vaw_adamw_ema_step_guarded(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                                          float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                          float bc2, float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad,
                                          const int32_t* ok, vaw_stream stream) {
    AdamArgs a{lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), ema_decay, clip_max_norm, zero_grad};
    return adamw_launch("adamw_ema_guarded", p, g, m, v, ema, shadow_bf16, n, nullptr, a, sumsq, ok, true, stream);
}

extern "C" int vaw_adamw_ema_step_guarded_dev(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                                              const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                                              float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad,
                                              const int32_t* ok, vaw_stream stream) {
    VAW_CHECK_ARG(hyper, "adamw_ema_guarded_dev: no hyper buffer");
    AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, ema_decay, clip_max_norm, zero_grad};
    return adamw_launch("adamw_ema_guarded_dev", p, g, m, v, ema, shadow_bf16, n, hyper, a, sumsq, ok, true, stream);
}

__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ src, int64_t n, float d) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        ema[i] = ema[i] * d + src[i] * (1.f - d);
}
extern "C" int vaw_ema_update(float* ema, const float* src, int64_t n, float decay, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "ema: n<=0");
    ema_kernel<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(ema, src, n, decay);
    VAW_CHECK_LAUNCH("ema");
    return VAW_OK;
}

__global__ void cast_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        store4(dst + 4 * i, load4(src + 4 * i));
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (bf16_t)src[i];
}
extern "C" int vaw_cast_bf16(const float* src, void* dst, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0, "cast_bf16: n<=0 or unaligned");
    cast_bf16_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(src, (bf16_t*)dst, n);
    VAW_CHECK_LAUNCH("cast_bf16");
    return VAW_OK;
}

// dst[i] = scale * float(src[i]): gradient buckets that travelled over xGMI in bf16 come back into the f32 gradient
// buffer (scale = 1/world when the collective summed instead of averaging).
__global__ void uncast_bf16_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t n, float scale) {
    const int64_t n8 = n / 8;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const bf16x8 v = reinterpret_cast<const bf16x8*>(src)[i];
        f32x4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
        reinterpret_cast<f32x4*>(dst)[2 * i] = a * scale;
        reinterpret_cast<f32x4*>(dst)[2 * i + 1] = b * scale;
    }
    for (int64_t i = n8 * 8 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = scale * (float)src[i];
}
extern "C" int vaw_uncast_bf16(const void* src, float* dst, int64_t n, float scale, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "uncast_bf16: n<=0 or unaligned");
    uncast_bf16_kernel<<<stream_grid(n / 8 + 1, 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)src, dst, n, scale);
    VAW_CHECK_LAUNCH("uncast_bf16");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Passes of the training step that replace a chain of tensor operations around the model (VAW_STEP_FUSED).  Every
// value is the one the chain produces: the same operations in the same order, each rounded on its own (-ffp-contract=off).
// ---------------------------------------------------------------------------------------------
// latent [B][2][n] = the VAE posterior's mean and std planes of a sample ->
//   x0  = (mean + std * eps) * scale                       (sample_from_latent: product, sum, product)
//   x_t = tab_a[t] * x0 + tab_s[t] * noise                  (mix_rows_kernel<true>)
//   tf[b] = float(t[b]) * t_scale                           (_scale_timesteps; optional)
__global__ void latent_qsample_kernel(const float* __restrict__ latent, const float* __restrict__ eps, const float* __restrict__ noise,
                                      const int64_t* __restrict__ t, const float* __restrict__ tab_a, const float* __restrict__ tab_s,
                                      int T, float scale, float t_scale, float* __restrict__ x0, float* __restrict__ x_t,
                                      float* __restrict__ tf, int64_t n) {
    const int b = blockIdx.y;
    float a, c;
    gather_mix_coef(tab_a, tab_s, t, T, b, a, c);
    if (tf && blockIdx.x == 0 && threadIdx.x == 0) tf[b] = (float)t[b] * t_scale;
    const float* mr = latent + (int64_t)b * 2 * n;
    const float* sr = mr + n;
    const float* er = eps + (int64_t)b * n;
    const float* nr = noise + (int64_t)b * n;
    float* xr = x0 + (int64_t)b * n;
    float* orow = x_t + (int64_t)b * n;
    const int64_t n4 = ((n & 3) == 0) ? n / 4 : 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 x = (load4(mr + 4 * i) + load4(sr + 4 * i) * load4(er + 4 * i)) * scale;
        store4(xr + 4 * i, x);
        store4(orow + 4 * i, a * x + c * load4(nr + 4 * i));
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = (mr[i] + sr[i] * er[i]) * scale;
        xr[i] = x;
        orow[i] = a * x + c * nr[i];
    }
}

extern "C" int vaw_latent_qsample(const float* latent, const float* eps, const float* noise, const int64_t* t, const float* tab_a,
                                  const float* tab_s, int num_timesteps, float latent_scale, float t_scale, float* x0, float* x_t,
                                  float* t_float, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && B <= 65535 && per_sample > 0 && num_timesteps > 0, "latent_qsample: bad sizes B=%d n=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(latent && eps && noise && t && tab_a && tab_s && x0 && x_t, "latent_qsample: null pointer");
    VAW_CHECK_ARG(per_sample % 4 != 0 || ((((uintptr_t)latent | (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)x0 | (uintptr_t)x_t) & 15) == 0),
                  "latent_qsample: tensors must be 16-byte aligned");
    int gx = stream_grid(per_sample / 4 + 1, 256);
    dim3 grid(gx > 64 ? 64 : gx, B);
    latent_qsample_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(latent, eps, noise, t, tab_a, tab_s, num_timesteps, latent_scale, t_scale,
                                                                x0, x_t, t_float, per_sample);
    VAW_CHECK_LAUNCH("latent_qsample");
    return VAW_OK;
}

extern "C" int vaw_wmse_fwd_t(const float* model_out, const float* x0, const float* noise, const int64_t* t, const float* ca,
                              const float* cb, const float* w, int num_timesteps, float* mse, float* mean_out, float accum, int B,
                              int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0 && (!t || num_timesteps > 0) && accum >= 1.f, "wmse_fwd_t: bad sizes");
    VAW_CHECK_ARG(model_out && x0 && noise && ca && cb && w && mse, "wmse_fwd_t: null pointer");
    wmse_fwd_t_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(model_out, x0, noise, ca, cb, w, t, num_timesteps, mse, per_sample,
                                                           vec4_ok(per_sample, 0, {model_out, x0, noise}));
    if (mean_out) batch_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(mse, B, accum, mean_out);
    VAW_CHECK_LAUNCH("wmse_fwd_t");
    return VAW_OK;
}

extern "C" int vaw_wmse_bwd_t(const float* model_out, const float* x0, const float* noise, const int64_t* t, const float* ca,
                              const float* cb, const float* w, int num_timesteps, const float* g, float inv_count, float* dout, int B,
                              int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && B <= 65535 && per_sample > 0 && (!t || num_timesteps > 0), "wmse_bwd_t: bad sizes");
    VAW_CHECK_ARG(model_out && x0 && noise && ca && cb && w && g && dout, "wmse_bwd_t: null pointer");
    int gx = stream_grid(per_sample / 4 + 1, 256);
    dim3 grid(gx > 64 ? 64 : gx, B);
    wmse_bwd_t_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(model_out, x0, noise, ca, cb, w, t, num_timesteps, g, 0, inv_count, dout,
                                                            per_sample, vec4_ok(per_sample, 0, {model_out, x0, noise, dout}));
    VAW_CHECK_LAUNCH("wmse_bwd_t");
    return VAW_OK;
}

// dst (bf16, row stride ld_dst) = src (f32 [M][N], row stride ld_src) and, in the same pass, colsum[n] = beta * colsum[n] +
// sum_m float(dst[m][n]): the sums of the values as stored, in the order vaw_colsum(VAW_BF16, dst, ...) adds them for M <= 512
// (colsum_partial_kernel<bf16_t>: four interleaved row groups, rows ascending inside a group, ((g0 + g1) + g2) + g3; then
// colsum_final_kernel over that one partial row: 0 + p, then beta * out + it) -- bitwise its result.  256 columns per workgroup,
// every lane CC_U independent 16-byte loads in flight.  The adaLN modulation gradient of dit.py: the cast feeds two GEMMs, the
// column sums are the bias gradient; separately they were three launches reading the tensor twice.
#define CC_U 16
__global__ void __launch_bounds__(256)
cast_colsum_kernel(const float* __restrict__ X, int64_t ldx, bf16_t* __restrict__ Y, int64_t ldy, int64_t M, int64_t N,
                   float* __restrict__ out, float beta) {
    __shared__ __attribute__((aligned(16))) float part[4][256];
    const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int64_t col = (int64_t)blockIdx.x * 256 + cg * 4;
    f32x4 acc = {0, 0, 0, 0};
    if (col < N) {          // N % 4 == 0: a group of 4 columns is in or out as a whole
        int64_t r = rg;
        for (; r + 4 * (CC_U - 1) < M; r += 4 * CC_U) {
            f32x4 v[CC_U];
#pragma unroll
            for (int u = 0; u < CC_U; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(X + (r + 4 * u) * ldx + col));
#pragma unroll
            for (int u = 0; u < CC_U; ++u) {          // rows ascending: fixed order
                bf16_t* y = Y + (r + 4 * u) * ldy + col;
                store4(y, v[u]);
                const bf16x4 q = {(bf16_t)v[u][0], (bf16_t)v[u][1], (bf16_t)v[u][2], (bf16_t)v[u][3]};
                acc += f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
            }
        }
        for (; r < M; r += 4) {
            const f32x4 v = load4(X + r * ldx + col);
            store4(Y + r * ldy + col, v);
            const bf16x4 q = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
            acc += f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
        }
    }
    store4(&part[rg][cg * 4], acc);
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < N) {
        const float p = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        float tsum = 0.f;
        tsum += p;
        out[c] = (beta != 0.f ? beta * out[c] : 0.f) + tsum;
    }
}

// host arithmetic only: the launch vaw_cast_colsum_bf16 makes, or why it makes none
extern "C" int vaw_cast_colsum_plan(int64_t M, int64_t N, int64_t ld_src, int64_t ld_dst, int64_t src_addr, int64_t dst_addr,
                                    int64_t colsum_addr, vaw_cast_colsum_launch* out) {
    VAW_CHECK_ARG(out != nullptr, "cast_colsum_plan: out is NULL");
    vaw_cast_colsum_launch p = {};
    *out = p;
    VAW_CHECK_ARG(M > 0 && N > 0 && ld_src >= N && ld_dst >= N, "cast_colsum: bad sizes M=%ld N=%ld ld_src=%ld ld_dst=%ld", (long)M, (long)N,
                  (long)ld_src, (long)ld_dst);
    // beyond 512 rows vaw_colsum cuts the rows into blocks (and takes another kernel for bf16 from 1024 on): another summation order
    VAW_CHECK_ARG(M <= 512, "cast_colsum: M=%ld > 512 rows is left to vaw_cast_bf16 + vaw_colsum", (long)M);
    VAW_CHECK_ARG(N % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0, "cast_colsum: N, ld_src and ld_dst must be multiples of 4");
    VAW_CHECK_ARG((src_addr & 15) == 0 && (dst_addr & 15) == 0 && (colsum_addr & 3) == 0 && src_addr && dst_addr && colsum_addr,
                  "cast_colsum: src and dst must be 16-byte aligned");
    VAW_CHECK_ARG((N + 255) / 256 < (1LL << 31), "cast_colsum: N too large");
    p.grid_x = (int)((N + 255) / 256);
    p.block = 256;
    p.rows_per_lane = (int)((M + 3) / 4);
    p.bytes_read = M * N * 4;
    p.bytes_written = M * N * 2 + N * 4;
    *out = p;
    return VAW_OK;
}

extern "C" int vaw_cast_colsum_bf16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t M, int64_t N, float* colsum,
                                    float beta, vaw_stream stream) {
    vaw_cast_colsum_launch p;
    const int rc = vaw_cast_colsum_plan(M, N, ld_src, ld_dst, (int64_t)(uintptr_t)src, (int64_t)(uintptr_t)dst, (int64_t)(uintptr_t)colsum, &p);
    if (rc != VAW_OK) return rc;
    cast_colsum_kernel<<<p.grid_x, p.block, 0, (hipStream_t)stream>>>(src, ld_src, (bf16_t*)dst, ld_dst, M, N, colsum, beta);
    VAW_CHECK_LAUNCH("cast_colsum_bf16");
    return VAW_OK;
}

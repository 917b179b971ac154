// Solver steps of the EDM (Euler / Heun, float64), linear multistep (DPM-Solver++ 2M / 2M-SDE / exponential Adams-Bashforth,
// float64) and flow-matching (SDE / ODE, float32) samplers: one streaming pass each around the denoiser call.  The coefficients of a step do not depend on x; they come from a device table built once per
// grid (samplers.py) and are read by row index.  Every operation is rounded on its own, in the order of the tensor
// composition these kernels replace (this file is built with -ffp-contract=off; divisions and square roots are IEEE).
// The model output of a guided call is the stacked [2N, ...] tensor read in place: rows model_ld floats apart.
// Each kernel has one loop body over per_sample / W items of W elements, W = 4 or 1 (common.h: loadw / storew, vec4_ok,
// VAW_LAUNCH_W, row_grid); the per-element work is the same inlined function at either width, so the two give the same bits.
#include "common.h"
#include "flow_fields.h"

// ---------------------------------------------------------------------------------------------
// EDM.  Table row (VAW_EDM_COLS doubles) of step i:
//   0 x_hat scale s(t_hat)/s(t_cur)   1 noise coefficient   2..9 evaluation at t_hat   10 h   11 alpha*h   12, 13 Heun weights
//   14..21 evaluation at t_mid.  An evaluation block: s(t), sigma as the denoiser sees it (f32), c_in, c_in^2, sigma*c_in
//   (the f32 scalars of EDMDenoiser.forward, stored widened), dsg/sg + ds/sc, dsg*sc/sg, chain index.
// ---------------------------------------------------------------------------------------------
struct EdmEval {
    double s, k1, k2;
    float sigma, cin, cin2, sc;
};
__device__ __forceinline__ EdmEval edm_eval(const double* r) {
    EdmEval e;
    e.s = r[0]; e.sigma = (float)r[1]; e.cin = (float)r[2]; e.cin2 = (float)r[3]; e.sc = (float)r[4]; e.k1 = r[5]; e.k2 = r[6];
    return e;
}
// f32 model input of EDMDenoiser.forward for the f64 state x at an evaluation: c_in * f32(x / s)
__device__ __forceinline__ float edm_model_in(const EdmEval& e, double x) { return e.cin * (float)(x / e.s); }
// the denoised image of EDMDenoiser.forward (pred: 0 EPSILON, 1 START_X, 2 VELOCITY) for model output o at the f32 state x32
__device__ __forceinline__ float edm_denoised(int pred, float sigma, float cin2, float sc, float x32, float o) {
    if (pred == 0) return x32 - sigma * o;
    if (pred == 1) return o;
    return cin2 * x32 - sc * o;
}
// dx/dt of _Path.slope with that denoised image
__device__ __forceinline__ double edm_slope(const EdmEval& e, int pred, double x, float o) {
    const float den = edm_denoised(pred, e.sigma, e.cin2, e.sc, (float)(x / e.s), o);
    return e.k1 * x - e.k2 * (double)den;
}

template <int W>
__global__ void edm_input_kernel(const double* __restrict__ x, const double* __restrict__ noise, const double* __restrict__ coef,
                                 double* __restrict__ x_hat, float* __restrict__ min, float* __restrict__ min2, int64_t n) {
    const double A = coef[0], nc = coef[1];
    const EdmEval e = edm_eval(coef + 2);
    const int64_t base = (int64_t)blockIdx.y * n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        double xv[W], nz[W];
        float mi[W];
        loadw<W>(x + o, xv);
        if (noise) loadw<W>(noise + o, nz);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            double h = A * xv[j];
            if (noise) h = h + nc * nz[j];
            xv[j] = h;
            mi[j] = edm_model_in(e, h);
        }
        storew<W>(x_hat + o, xv);
        storew<W>(min + o, mi);
        if (min2) storew<W>(min2 + o, mi);
    }
}

extern "C" int vaw_edm_input(const double* x, const double* noise, const double* coef, int row, int rows, double* x_hat,
                             float* model_in, float* model_in_dup, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "edm_input: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(x && coef && x_hat && model_in, "edm_input: null pointer");
    VAW_CHECK_ARG(row >= 0 && row < rows, "edm_input: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)noise & 7) == 0 && ((uintptr_t)x_hat & 7) == 0 && ((uintptr_t)coef & 7) == 0,
                  "edm_input: float64 pointer not aligned to 8 bytes");
    const bool vec = vec4_ok(per_sample, 0, {x, noise, x_hat, model_in, model_in_dup});
    VAW_LAUNCH_W(edm_input_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, x, noise,
                 coef + (int64_t)row * VAW_EDM_COLS, x_hat, model_in, model_in_dup, per_sample);
    VAW_CHECK_LAUNCH("edm_input");
    return VAW_OK;
}

// kind 0 Euler:         x_out = x_hat + h * d,                      d = slope(x_hat, t_hat)
// kind 1 Heun predict:  d_cur = d;  x_mid = x_hat + (alpha h) * d;  model input of x_mid at t_mid
// kind 2 Heun correct:  x_mid recomputed from x_hat and d_cur (the same two operations, so the same bits);
//                       d' = slope(x_mid, t_mid);  x_out = x_hat + h * (w1 * d_cur + w2 * d')
struct EdmStepArgs {
    const float *cond, *uncond;
    int64_t ld;
    float gs;
    const double *x_hat, *coef;
    double *d_cur, *x_out;
    float *min, *min2;
    int64_t n;
    int kind, pred;
};

__device__ __forceinline__ void edm_step_elem(int kind, int pred, const EdmEval& hat, const EdmEval& mid, double h, double ah, double w1,
                                              double w2, double xh, float o, double& dc, double& xo, float& mi) {
    if (kind == 2) {
        const double xm = xh + ah * dc;
        const double dm = edm_slope(mid, pred, xm, o);
        xo = xh + h * (w1 * dc + w2 * dm);
        return;
    }
    const double d = edm_slope(hat, pred, xh, o);
    if (kind == 0) {
        xo = xh + h * d;
        return;
    }
    dc = d;
    mi = edm_model_in(mid, xh + ah * d);
}

template <int W>
__global__ void edm_step_kernel(const EdmStepArgs a) {
    const double* r = a.coef;
    const EdmEval hat = edm_eval(r + 2), mid = edm_eval(r + 14);
    const double h = r[10], ah = r[11], w1 = r[12], w2 = r[13];
    const int kind = a.kind, pred = a.pred;
    const int64_t n = a.n, base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * a.ld;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        double xh[W], dc[W], xo[W];
        float c[W], u[W], mi[W];
        loadw<W>(a.x_hat + o, xh);
        loadw<W>(a.cond + mbase + W * i, c);
        if (a.uncond) loadw<W>(a.uncond + mbase + W * i, u);
        if (kind == 2) loadw<W>(a.d_cur + o, dc);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float m = a.uncond ? cfg_mix(c[j], u[j], a.gs) : c[j];
            edm_step_elem(kind, pred, hat, mid, h, ah, w1, w2, xh[j], m, dc[j], xo[j], mi[j]);
        }
        if (kind == 1) {
            storew<W>(a.d_cur + o, dc);
            storew<W>(a.min + o, mi);
            if (a.min2) storew<W>(a.min2 + o, mi);
        } else {
            storew<W>(a.x_out + o, xo);
        }
    }
}

extern "C" int vaw_edm_step(int kind, int pred_type, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                            const double* x_hat, double* d_cur, const double* coef, int row, int rows, double* x_out,
                            float* model_in, float* model_in_dup, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "edm_step: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(kind >= 0 && kind <= 2 && pred_type >= 0 && pred_type <= 2, "edm_step: bad kind %d or pred_type %d", kind, pred_type);
    VAW_CHECK_ARG(cond && x_hat && coef, "edm_step: null pointer");
    VAW_CHECK_ARG(kind == 1 ? (d_cur && model_in) : (x_out && (kind == 0 || d_cur)),
                  "edm_step: kind 1 needs d_cur and model_in, kind 0 x_out, kind 2 d_cur and x_out");
    VAW_CHECK_ARG(model_ld >= per_sample, "edm_step: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG(row >= 0 && row < rows, "edm_step: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(((uintptr_t)x_hat & 7) == 0 && ((uintptr_t)d_cur & 7) == 0 && ((uintptr_t)x_out & 7) == 0 && ((uintptr_t)coef & 7) == 0,
                  "edm_step: float64 pointer not aligned to 8 bytes");
    if (kind == 0) d_cur = nullptr;
    if (kind == 1) x_out = nullptr;
    else model_in = model_in_dup = nullptr;
    const bool vec = vec4_ok(per_sample, model_ld, {cond, uncond, x_hat, d_cur, x_out, model_in, model_in_dup});
    const EdmStepArgs a = {cond, uncond, model_ld, guidance_scale, x_hat, coef + (int64_t)row * VAW_EDM_COLS, d_cur, x_out,
                           model_in, model_in_dup, per_sample, kind, pred_type};
    VAW_LAUNCH_W(edm_step_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, a);
    VAW_CHECK_LAUNCH("edm_step");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Linear multistep samplers (dpm_sample).  Table row (VAW_DPM_COLS doubles) of step i:
//   0 a  1 b0  2 b1  3 b2  4 c  of  x' = a x + b0 D0 + b1 D1 + b2 D2 + c noise;  5 sigma (f32)  6 c_in  7 c_in^2  8 sigma*c_in of
//   this evaluation (the f32 scalars of EDMDenoiser.forward, stored widened);  9 c_in of the next evaluation.
// The denoised images D0, D1, D2 are f32 values and stay f32 in memory; the state is f64.
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ void dpm_input_kernel(const double* __restrict__ x, const double* __restrict__ coef, float* __restrict__ min,
                                 float* __restrict__ min2, int64_t n) {
    const float cin = (float)coef[6];
    const int64_t base = (int64_t)blockIdx.y * n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        double xv[W];
        float mi[W];
        loadw<W>(x + o, xv);
#pragma unroll
        for (int j = 0; j < W; ++j) mi[j] = cin * (float)xv[j];
        storew<W>(min + o, mi);
        if (min2) storew<W>(min2 + o, mi);
    }
}

extern "C" int vaw_dpm_input(const double* x, const double* coef, int row, int rows, float* model_in, float* model_in_dup, int B,
                             int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "dpm_input: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(x && coef && model_in, "dpm_input: null pointer");
    VAW_CHECK_ARG(row >= 0 && row < rows, "dpm_input: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)coef & 7) == 0, "dpm_input: float64 pointer not aligned to 8 bytes");
    const bool vec = vec4_ok(per_sample, 0, {x, model_in, model_in_dup});
    VAW_LAUNCH_W(dpm_input_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, x,
                 coef + (int64_t)row * VAW_DPM_COLS, model_in, model_in_dup, per_sample);
    VAW_CHECK_LAUNCH("dpm_input");
    return VAW_OK;
}

// x_out may be x (no __restrict__ on either): a lane loads its W elements of every input before it stores any
struct DpmStepArgs {
    const float *cond, *uncond;
    int64_t ld;
    float gs;
    const double *x, *noise, *coef;
    const float *d1, *d2;
    double* x_out;
    float *d0_out, *min, *min2;
    int64_t n;
    int pred, clip;
};

template <int W>
__global__ void dpm_step_kernel(const DpmStepArgs a) {
    const double* r = a.coef;
    const double ca = r[0], b0 = r[1], b1 = r[2], b2 = r[3], cn = r[4];
    const float sigma = (float)r[5], cin2 = (float)r[7], sc = (float)r[8], cin_next = (float)r[9];
    const int pred = a.pred;
    const bool clip = a.clip != 0;
    const int64_t n = a.n, base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * a.ld;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        double xv[W], nz[W];
        float c[W], u[W], p1[W], p2[W], d0[W], mi[W];
        loadw<W>(a.x + o, xv);
        loadw<W>(a.cond + mbase + W * i, c);
        if (a.uncond) loadw<W>(a.uncond + mbase + W * i, u);
        if (a.d1) loadw<W>(a.d1 + o, p1);
        if (a.d2) loadw<W>(a.d2 + o, p2);
        if (a.noise) loadw<W>(a.noise + o, nz);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float m = a.uncond ? cfg_mix(c[j], u[j], a.gs) : c[j];
            float den = edm_denoised(pred, sigma, cin2, sc, (float)xv[j], m);
            if (clip) den = den < -1.f ? -1.f : (den > 1.f ? 1.f : den);          // torch.clamp: NaN stays NaN
            d0[j] = den;
            double acc = ca * xv[j] + b0 * (double)den;
            if (a.d1) acc = acc + b1 * (double)p1[j];
            if (a.d2) acc = acc + b2 * (double)p2[j];
            if (a.noise) acc = acc + cn * nz[j];
            xv[j] = acc;
            mi[j] = cin_next * (float)acc;
        }
        storew<W>(a.d0_out + o, d0);
        storew<W>(a.x_out + o, xv);
        if (a.min) storew<W>(a.min + o, mi);
        if (a.min2) storew<W>(a.min2 + o, mi);
    }
}

extern "C" int vaw_dpm_step(int pred_type, int clip, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                            const double* x, const float* d1, const float* d2, const double* noise, const double* coef, int row,
                            int rows, double* x_out, float* d0_out, float* model_in, float* model_in_dup, int B, int64_t per_sample,
                            vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "dpm_step: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(pred_type >= 0 && pred_type <= 2, "dpm_step: bad pred_type %d", pred_type);
    VAW_CHECK_ARG(cond && x && coef && x_out && d0_out, "dpm_step: null pointer");
    VAW_CHECK_ARG(d1 || !d2, "dpm_step: d2 (the third node) needs d1");
    VAW_CHECK_ARG(model_in || !model_in_dup, "dpm_step: model_in_dup needs model_in");
    VAW_CHECK_ARG(model_ld >= per_sample, "dpm_step: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG(row >= 0 && row < rows, "dpm_step: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)noise & 7) == 0 && ((uintptr_t)x_out & 7) == 0 && ((uintptr_t)coef & 7) == 0,
                  "dpm_step: float64 pointer not aligned to 8 bytes");
    const bool vec = vec4_ok(per_sample, model_ld, {cond, uncond, x, d1, d2, noise, x_out, d0_out, model_in, model_in_dup});
    const DpmStepArgs a = {cond, uncond, model_ld, guidance_scale, x, noise, coef + (int64_t)row * VAW_DPM_COLS, d1, d2, x_out,
                           d0_out, model_in, model_in_dup, per_sample, pred_type, clip};
    VAW_LAUNCH_W(dpm_step_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, a);
    VAW_CHECK_LAUNCH("dpm_step");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Flow matching.  Table row (VAW_FLOW_COLS floats) of one evaluation at time t:
//   0 a  1 s  2 a'  3 s'  4 g2 = 2 s s'  5 g2/2  6 s^2  7 a^2 + s^2  8 s a' - a s'  9 sqrt(g2)
//   and of the step that starts there:  10 dt  11 sqrt(|dt|)  12 dt/2  (13 t).
// FlowRow / flow_row / flow_drift: flow_fields.h (shared with the adaptive stages of ode_adaptive.hip).
// ---------------------------------------------------------------------------------------------
// kind 0 Euler:         x_out = (x + f0 dt) + kick           (kick = (sqrt(g2) noise) sqrt|dt|; none without noise, none for the ODE)
// kind 1 Heun predict:  f0, kick stored;  x_out = the Euler step (the input of the second evaluation)
// kind 2 Heun correct:  f1 = drift(x_pred, row1);  SDE x_out = (x + (0.5 (f0 + f1)) dt) + kick,  ODE x_out = x + (dt/2)(f0 + f1)
struct FlowStepArgs {
    const float *cond, *uncond;
    int64_t ld;
    float gs;
    const float *x, *noise, *x_pred, *r0, *r1;
    float *f0, *kick, *x_out, *x_out2;
    int64_t n;
    int kind, sde, mt;
};

__device__ __forceinline__ float flow_step_elem(const FlowStepArgs& a, const FlowRow& e0, const FlowRow& e1, float sg2, float dt, float sdt,
                                                float hdt, float o, float x, float nz, float xp, float& f0, float& kick) {
    const bool sde = a.sde != 0;
    if (a.kind == 2) {
        const float f1 = flow_drift(e1, a.mt, sde, o, xp);
        if (sde) {
            const float y = x + (0.5f * (f0 + f1)) * dt;
            return a.kick ? y + kick : y;
        }
        return x + hdt * (f0 + f1);
    }
    f0 = flow_drift(e0, a.mt, sde, o, x);
    const float y = x + f0 * dt;
    if (!a.noise) return y;
    kick = (sg2 * nz) * sdt;
    return y + kick;
}

template <int W>
__global__ void flow_step_kernel(const FlowStepArgs a) {
    const FlowRow e0 = flow_row(a.r0), e1 = flow_row(a.r1);
    const float sg2 = a.r0[9], dt = a.r0[10], sdt = a.r0[11], hdt = a.r0[12];
    const int64_t n = a.n, base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * a.ld;
    const bool corr = a.kind == 2, pred = a.kind == 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        float c[W], u[W], x[W], nz[W] = {}, xp[W] = {}, f0[W], kk[W] = {}, y[W];
        loadw<W>(a.cond + mbase + W * i, c);
        if (a.uncond) loadw<W>(a.uncond + mbase + W * i, u);
        loadw<W>(a.x + o, x);
        if (!corr && a.noise) loadw<W>(a.noise + o, nz);
        if (corr) {
            loadw<W>(a.x_pred + o, xp);
            loadw<W>(a.f0 + o, f0);
            if (a.kick) loadw<W>(a.kick + o, kk);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float m = a.uncond ? cfg_mix(c[j], u[j], a.gs) : c[j];
            y[j] = flow_step_elem(a, e0, e1, sg2, dt, sdt, hdt, m, x[j], nz[j], xp[j], f0[j], kk[j]);
        }
        if (pred) {
            storew<W>(a.f0 + o, f0);
            if (a.kick) storew<W>(a.kick + o, kk);
        }
        storew<W>(a.x_out + o, y);
        if (a.x_out2) storew<W>(a.x_out2 + o, y);
    }
}

extern "C" int vaw_flow_step(int kind, int sde, int mean_type, const float* cond, const float* uncond, int64_t model_ld,
                             float guidance_scale, const float* x, const float* noise, const float* x_pred, float* f0, float* kick,
                             const float* coef, int row0, int row1, int rows, float* x_out, float* x_out_dup, int B,
                             int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "flow_step: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(kind >= 0 && kind <= 2 && mean_type >= 0 && mean_type <= 3 && (sde == 0 || sde == 1),
                  "flow_step: bad kind %d, mean_type %d or sde %d", kind, mean_type, sde);
    VAW_CHECK_ARG(cond && x && coef && x_out, "flow_step: null pointer");
    VAW_CHECK_ARG(kind == 0 || f0, "flow_step: Heun steps need f0");
    VAW_CHECK_ARG(kind != 2 || x_pred, "flow_step: the Heun correction needs x_pred");
    VAW_CHECK_ARG(sde || !(noise || kick), "flow_step: the ODE takes no noise");
    VAW_CHECK_ARG(kind != 1 || !sde || (!noise == !kick), "flow_step: an SDE Heun prediction stores the kick of its noise");
    VAW_CHECK_ARG(model_ld >= per_sample, "flow_step: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG(row0 >= 0 && row0 < rows && row1 >= 0 && row1 < rows, "flow_step: rows %d, %d outside the table of %d rows", row0, row1,
                  rows);
    if (kind == 0) f0 = kick = nullptr;
    if (kind == 2) noise = nullptr;
    else x_pred = nullptr;
    const bool vec = vec4_ok(per_sample, model_ld, {cond, uncond, x, noise, x_pred, f0, kick, x_out, x_out_dup});
    const FlowStepArgs a = {cond, uncond, model_ld, guidance_scale, x, noise, x_pred, coef + (int64_t)row0 * VAW_FLOW_COLS,
                            coef + (int64_t)row1 * VAW_FLOW_COLS, f0, kick, x_out, x_out_dup, per_sample, kind, sde, mean_type};
    VAW_LAUNCH_W(flow_step_kernel, vec, row_grid(vec ? per_sample / 4 : per_sample, B), 256, stream, a);
    VAW_CHECK_LAUNCH("flow_step");
    return VAW_OK;
}

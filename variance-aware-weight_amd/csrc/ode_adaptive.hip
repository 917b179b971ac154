// Adaptive explicit Runge-Kutta integration of the flow ODE (samplers.py: flow_ode_sample(solver="rk45")): the streaming pass
// after each network evaluation of a step, and the scaled sums of squares the step controller on the host decides by.
// Conventions of solver_steps.hip: float32 state, every operation rounded on its own in the order of the tensor composition
// (built with -ffp-contract=off; IEEE division), the model output read in place (cond / uncond rows model_ld apart, combined
// as vaw_cfg_combine does), one loop body at W = 4 (16-byte accesses) and W = 1.  No atomics, no allocation, no host
// synchronisation: a sum leaves the kernel as one float64 partial per workgroup, folded in a fixed order, so its bits do not
// change from run to run.
#include "common.h"
#include "flow_fields.h"

// One grid row per sample and one workgroup per 1024 elements of it, at most VAW_RK_MAX_GRID_X (grid-stride beyond), at either
// width: the number of partial sums depends on the sizes alone (vaw_rk_partial_count), not on the alignment of the pointers.
static inline dim3 rk_grid(int64_t per_sample, int B) {
    int64_t g = (per_sample + 1023) / 1024;
    return dim3((unsigned)(g < 1 ? 1 : (g > VAW_RK_MAX_GRID_X ? VAW_RK_MAX_GRID_X : g)), (unsigned)B);
}

extern "C" int64_t vaw_rk_partial_count(int B, int64_t per_sample) {
    if (B <= 0 || per_sample <= 0) return 0;
    return (int64_t)rk_grid(per_sample, B).x * B;
}

// The workgroup's sum of `acc` in a fixed order (butterfly within a wave, waves in order) -> partials[workgroup].
__device__ __forceinline__ void rk_block_partial(double acc, double* partials) {
    __shared__ double waves[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

// max(|a|, |b|) as torch.maximum gives it: a NaN on either side stays a NaN
__device__ __forceinline__ float rk_absmax(float a, float b) {
    return (a != a || b != b) ? __builtin_nanf("") : fmaxf(fabsf(a), fabsf(b));
}

struct RkStageArgs {
    const float *cond, *uncond;
    int64_t ld;
    float gs;
    const float *x, *x_stage, *x_new, *row;
    float* k;
    int64_t kstride;
    float *x_out, *x_out2;
    double* partials;
    float h, atol, rtol;
    float a[VAW_RK_STAGES];
    int slot[VAW_RK_STAGES];
    int ncoef, stage, mt;
    int64_t n;
};

template <int W>
__global__ void __launch_bounds__(256) rk_stage_kernel(const RkStageArgs a) {
    FlowRow f = {};
    if (a.cond) f = flow_row(a.row);          // (without a network output there is no table row: a.row is null)
    const int64_t n = a.n, base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * a.ld;
    float* const ki = a.k + a.slot[a.stage] * a.kstride;
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        float kv[W], dy[W] = {};
        if (a.cond) {          // k_stage from the network output at the stage's own state
            float c[W], u[W], xs[W];
            loadw<W>(a.cond + mbase + W * i, c);
            if (a.uncond) loadw<W>(a.uncond + mbase + W * i, u);
            loadw<W>(a.x_stage + o, xs);
#pragma unroll
            for (int j = 0; j < W; ++j) kv[j] = flow_drift(f, a.mt, false, a.uncond ? cfg_mix(c[j], u[j], a.gs) : c[j], xs[j]);
            storew<W>(ki + o, kv);
        }
        if (a.ncoef == 0) continue;
        bool first = true;          // dy = sum_s a_s k_s: ascending, zero coefficients skipped, left to right
#pragma unroll
        for (int s = 0; s < VAW_RK_STAGES; ++s) {
            if (s >= a.ncoef || a.a[s] == 0.f) continue;
            float t[W];
            if (s == a.stage && a.cond) {
#pragma unroll
                for (int j = 0; j < W; ++j) t[j] = kv[j];
            } else {
                loadw<W>(a.k + a.slot[s] * a.kstride + o, t);
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float p = a.a[s] * t[j];
                dy[j] = first ? p : dy[j] + p;
            }
            first = false;
        }
        float x[W];
        loadw<W>(a.x + o, x);
        if (a.partials) {          // the step's error against its tolerance
            float xn[W];
            loadw<W>(a.x_new + o, xn);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float err = a.h * dy[j];
                const float scale = a.atol + a.rtol * rk_absmax(x[j], xn[j]);
                const double r = (double)(err / scale);
                acc = acc + r * r;
            }
        } else {                   // the next stage's state, straight into the network's input
            float y[W];
#pragma unroll
            for (int j = 0; j < W; ++j) y[j] = x[j] + a.h * dy[j];
            storew<W>(a.x_out + o, y);
            if (a.x_out2) storew<W>(a.x_out2 + o, y);
        }
    }
    if (a.partials) rk_block_partial(acc, a.partials);
}

extern "C" int vaw_rk_stage(int stage, int mean_type, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                            const float* x, const float* x_stage, const float* coef, int row, int rows, float* k, const int* slots,
                            const float* a, int ncoef, float h, float* x_out, float* x_out_dup, const float* x_new, float atol,
                            float rtol, double* partials, int64_t partials_cap, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "rk_stage: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(stage >= 0 && stage < VAW_RK_STAGES && mean_type >= 0 && mean_type <= 3, "rk_stage: bad stage %d or mean_type %d", stage,
                  mean_type);
    VAW_CHECK_ARG(ncoef >= 0 && ncoef <= VAW_RK_STAGES, "rk_stage: %d coefficients (0..%d)", ncoef, VAW_RK_STAGES);
    VAW_CHECK_ARG(x && k && slots && (a || ncoef == 0), "rk_stage: null pointer");
    VAW_CHECK_ARG(cond || !uncond, "rk_stage: uncond without cond");
    VAW_CHECK_ARG(cond || ncoef > 0, "rk_stage: nothing to do (no network output and no coefficients)");
    VAW_CHECK_ARG(!cond || (coef && row >= 0 && row < rows), "rk_stage: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(!cond || model_ld >= per_sample, "rk_stage: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    for (int s = 0; s < VAW_RK_STAGES; ++s)
        VAW_CHECK_ARG(slots[s] >= 0 && slots[s] < VAW_RK_STAGES, "rk_stage: slot %d of stage %d outside the %d slots", slots[s], s, VAW_RK_STAGES);
    if (ncoef == 0) {
        VAW_CHECK_ARG(!x_out && !x_out_dup && !partials, "rk_stage: an output without coefficients");
    } else if (partials) {
        VAW_CHECK_ARG(x_new && !x_out && !x_out_dup, "rk_stage: the error needs x_new and writes no state");
        VAW_CHECK_ARG(((uintptr_t)partials & 7) == 0, "rk_stage: float64 pointer not aligned to 8 bytes");
        VAW_CHECK_ARG(partials_cap >= vaw_rk_partial_count(B, per_sample), "rk_stage: %ld partial sums do not fit %ld", (long)vaw_rk_partial_count(B, per_sample),
                      (long)partials_cap);
    } else {
        VAW_CHECK_ARG(x_out, "rk_stage: coefficients without x_out or partials");
    }
    if (!cond) x_stage = nullptr, coef = nullptr;
    else if (!x_stage) x_stage = x;
    if (!partials) x_new = nullptr;
    RkStageArgs g = {};
    g.cond = cond; g.uncond = uncond; g.ld = cond ? model_ld : per_sample; g.gs = guidance_scale;
    g.x = x; g.x_stage = x_stage; g.x_new = x_new; g.row = cond ? coef + (int64_t)row * VAW_FLOW_COLS : nullptr;
    g.k = k; g.kstride = (int64_t)B * per_sample; g.x_out = x_out; g.x_out2 = x_out_dup; g.partials = partials;
    g.h = h; g.atol = atol; g.rtol = rtol; g.ncoef = ncoef; g.stage = stage; g.mt = mean_type; g.n = per_sample;
    for (int s = 0; s < VAW_RK_STAGES; ++s) {
        g.a[s] = s < ncoef ? a[s] : 0.f;
        g.slot[s] = slots[s];
    }
    const bool vec = vec4_ok(per_sample, g.ld, {cond, uncond, x, x_stage, x_new, k, x_out, x_out_dup});
    VAW_LAUNCH_W(rk_stage_kernel, vec, rk_grid(per_sample, B), 256, stream, g);
    VAW_CHECK_LAUNCH("rk_stage");
    return VAW_OK;
}

// sum ((u - v) / (atol + rtol * max(|a|, |b|)))^2: the quotient in float32, its square and the sum in float64
template <int W>
__global__ void __launch_bounds__(256) rk_scaled_sumsq_kernel(const float* u, const float* v, const float* a, const float* b, float atol,
                                                              float rtol, double* partials, int64_t n) {
    const int64_t base = (int64_t)blockIdx.y * n;
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / W; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = base + W * i;
        float uv[W], vv[W], av[W], bv[W];
        loadw<W>(u + o, uv);
        if (v) loadw<W>(v + o, vv);
        loadw<W>(a + o, av);
        if (b) loadw<W>(b + o, bv);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float d = v ? uv[j] - vv[j] : uv[j];
            const float m = b ? rk_absmax(av[j], bv[j]) : fabsf(av[j]);
            const double r = (double)(d / (atol + rtol * m));
            acc = acc + r * r;
        }
    }
    rk_block_partial(acc, partials);
}

extern "C" int vaw_rk_scaled_sumsq(const float* u, const float* v, const float* a, const float* b, float atol, float rtol,
                                   double* partials, int64_t partials_cap, int B, int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "rk_scaled_sumsq: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(u && a && partials, "rk_scaled_sumsq: null pointer");
    VAW_CHECK_ARG(((uintptr_t)partials & 7) == 0, "rk_scaled_sumsq: float64 pointer not aligned to 8 bytes");
    VAW_CHECK_ARG(partials_cap >= vaw_rk_partial_count(B, per_sample), "rk_scaled_sumsq: %ld partial sums do not fit %ld",
                  (long)vaw_rk_partial_count(B, per_sample), (long)partials_cap);
    const bool vec = vec4_ok(per_sample, 0, {u, v, a, b});
    VAW_LAUNCH_W(rk_scaled_sumsq_kernel, vec, rk_grid(per_sample, B), 256, stream, u, v, a, b, atol, rtol, partials, per_sample);
    VAW_CHECK_LAUNCH("rk_scaled_sumsq");
    return VAW_OK;
}

// One workgroup folds `count` partial sums into out[0]: thread t takes t, t + 256, ... in order, then the fixed tree.
__global__ void __launch_bounds__(256) rk_sumsq_finish_kernel(const double* partials, int64_t count, double* out) {
    __shared__ double waves[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc = acc + partials[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

extern "C" int vaw_rk_sumsq_finish(const double* partials, int64_t count, double* out, vaw_stream stream) {
    VAW_CHECK_ARG(partials && out && count > 0, "rk_sumsq_finish: null pointer or no partial sums (%ld)", (long)count);
    VAW_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)out & 7) == 0, "rk_sumsq_finish: float64 pointer not aligned to 8 bytes");
    rk_sumsq_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials, count, out);
    VAW_CHECK_LAUNCH("rk_sumsq_finish");
    return VAW_OK;
}

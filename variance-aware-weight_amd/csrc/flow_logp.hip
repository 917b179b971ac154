// Log-likelihood of a flow model along its probability-flow ODE (samplers.py: flow_log_likelihood): the streaming pass after
// the network evaluation and the vector-Jacobian product of a Runge-Kutta stage, and the Gaussian prior at the far end.
// Conventions of ode_adaptive.hip: float32 state, every operation rounded on its own in the order of the tensor composition
// (built with -ffp-contract=off), the model output read in place by row stride, plain vector stores, no atomics, no
// allocation, no host synchronisation.  The divergence is float64: each product eps * g is exact there, and the sum runs in
// an order that depends on the per-sample size alone -- a thread takes whole quads of four consecutive elements (one 16-byte
// load each where rows are aligned, four scalar loads with a bound check otherwise: the same elements either way), a
// workgroup sums its 256 threads in a fixed tree, and a row that spans several workgroups leaves one partial per workgroup
// (vaw_rk_partial_count of them) that a second launch folds left to right.  So a row's bits do not depend on the batch, on
// the alignment of the pointers or on the run.
#include "common.h"

#define LN_2PI 1.8378770664093453

static inline dim3 logp_grid(int64_t per_sample, int B) {          // the grid vaw_rk_partial_count counts
    int64_t g = (per_sample + 1023) / 1024;
    return dim3((unsigned)(g < 1 ? 1 : (g > VAW_RK_MAX_GRID_X ? VAW_RK_MAX_GRID_X : g)), (unsigned)B);
}

// one quad of a row: elements i0 .. i0 + 3, those at or beyond n read as zero and are never written
template <bool VEC> __device__ __forceinline__ void ldq(const float* p, int64_t i0, int64_t n, float* v) {
    if constexpr (VEC) {
        loadw<4>(p + i0, v);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? p[i0 + j] : 0.f;
    }
}
template <bool VEC> __device__ __forceinline__ void stq(float* p, int64_t i0, int64_t n, const float* v) {
    if constexpr (VEC) {
        storew<4>(p + i0, v);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) p[i0 + j] = v[j];
    }
}

// The workgroup's sum of `acc` (butterfly within a wave, waves in order), valid in thread 0.
__device__ __forceinline__ double logp_block_sum(double acc) {
    __shared__ double waves[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

struct LogpStageArgs {
    const float *out, *g, *eps, *x, *x_stage, *row;
    int64_t ld, n, kstride;
    float *k, *x_out;
    double *d, *delta, *partials;
    double ad[VAW_RK_STAGES], hd;
    float a[VAW_RK_STAGES], h;
    int ncoef, stage, B;
};

// Row b's divergence from its sum of eps * g, and on the last stage the step's contribution to the accumulator.
__device__ __forceinline__ void logp_stage_finish(const LogpStageArgs& a, int b, double sum) {
    const double dv = (double)a.row[0] * (double)a.n + (double)a.row[1] * sum;
    a.d[(int64_t)a.stage * a.B + b] = dv;
    if (!a.delta) return;
    double acc = 0.0;          // sum_s b_s d_s: ascending, zero weights skipped, left to right
    bool first = true;
    for (int s = 0; s < a.ncoef; ++s) {
        if (a.ad[s] == 0.0) continue;
        const double p = a.ad[s] * (s == a.stage ? dv : a.d[(int64_t)s * a.B + b]);
        acc = first ? p : acc + p;
        first = false;
    }
    a.delta[b] = a.delta[b] + a.hd * acc;
}

template <int W>          // W = 4: 16-byte accesses, W = 1: scalar ones; the element-to-thread map is the same
__global__ void __launch_bounds__(256) flow_logp_stage_kernel(const LogpStageArgs a) {
    constexpr bool VEC = W == 4;
    const float A = a.row[0], Bc = a.row[1];
    const int64_t n = a.n, base = (int64_t)blockIdx.y * n, mbase = (int64_t)blockIdx.y * a.ld;
    float* const ki = a.k + a.stage * a.kstride + base;
    double acc = 0.0;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; 4 * q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = 4 * q;
        float o[4], xs[4], gv[4], ev[4], kv[4], dy[4] = {};
        ldq<VEC>(a.out + mbase, i0, n, o);
        ldq<VEC>(a.x_stage + base, i0, n, xs);
        ldq<VEC>(a.g + base, i0, n, gv);
        ldq<VEC>(a.eps + base, i0, n, ev);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kv[j] = A * xs[j] + Bc * o[j];
            acc = acc + (double)ev[j] * (double)gv[j];          // (elements beyond n were read as zero)
        }
        stq<VEC>(ki, i0, n, kv);
        if (a.ncoef == 0) continue;
        bool first = true;          // dy = sum_s a_s k_s: ascending, zero coefficients skipped, left to right
#pragma unroll
        for (int s = 0; s < VAW_RK_STAGES; ++s) {
            if (s >= a.ncoef || a.a[s] == 0.f) continue;
            float t[4];
            if (s == a.stage) {
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = kv[j];
            } else {
                ldq<VEC>(a.k + s * a.kstride + base, i0, n, t);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p = a.a[s] * t[j];
                dy[j] = first ? p : dy[j] + p;
            }
            first = false;
        }
        float x[4], y[4];
        ldq<VEC>(a.x + base, i0, n, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = x[j] + a.h * dy[j];
        stq<VEC>(a.x_out + base, i0, n, y);
    }
    const double sum = logp_block_sum(acc);
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) logp_stage_finish(a, blockIdx.y, sum);
    else a.partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// rows that span `gx` > 1 workgroups: one thread per row folds its partials left to right
__global__ void __launch_bounds__(256) flow_logp_stage_fold_kernel(const LogpStageArgs a, int gx) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    double sum = a.partials[(int64_t)b * gx];
    for (int i = 1; i < gx; ++i) sum = sum + a.partials[(int64_t)b * gx + i];
    logp_stage_finish(a, b, sum);
}

extern "C" int vaw_flow_logp_stage(int stage, const float* out, int64_t model_ld, const float* g, const float* eps, const float* x,
                                   const float* x_stage, const float* coef, int row, int rows, float* k, double* d, const double* a,
                                   int ncoef, double h, float* x_out, double* delta, double* partials, int64_t partials_cap, int B,
                                   int64_t per_sample, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "flow_logp_stage: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(stage >= 0 && stage < VAW_RK_STAGES, "flow_logp_stage: stage %d outside 0..%d", stage, VAW_RK_STAGES - 1);
    VAW_CHECK_ARG(ncoef >= 0 && ncoef <= VAW_RK_STAGES, "flow_logp_stage: %d coefficients (0..%d)", ncoef, VAW_RK_STAGES);
    VAW_CHECK_ARG(out && g && eps && x && coef && k && d && (a || ncoef == 0), "flow_logp_stage: null pointer");
    VAW_CHECK_ARG(row >= 0 && row < rows, "flow_logp_stage: row %d outside the table of %d rows", row, rows);
    VAW_CHECK_ARG(model_ld >= per_sample, "flow_logp_stage: model_ld %ld < per_sample %ld", (long)model_ld, (long)per_sample);
    VAW_CHECK_ARG((ncoef > 0) == (x_out != nullptr), "flow_logp_stage: coefficients and x_out come together");
    VAW_CHECK_ARG(!delta || ncoef > 0, "flow_logp_stage: the accumulator needs the step's weights");
    VAW_CHECK_ARG(((uintptr_t)d & 7) == 0 && ((uintptr_t)delta & 7) == 0 && ((uintptr_t)partials & 7) == 0,
                  "flow_logp_stage: float64 pointer not aligned to 8 bytes");
    const dim3 grid = logp_grid(per_sample, B);
    VAW_CHECK_ARG(grid.x == 1 || (partials && partials_cap >= (int64_t)grid.x * B), "flow_logp_stage: %ld partial sums do not fit %ld",
                  (long)grid.x * B, (long)partials_cap);
    LogpStageArgs p = {};
    p.out = out; p.g = g; p.eps = eps; p.x = x; p.x_stage = x_stage ? x_stage : x; p.row = coef + (int64_t)row * VAW_FLOW_LOGP_COLS;
    p.ld = model_ld; p.n = per_sample; p.kstride = (int64_t)B * per_sample; p.k = k; p.x_out = x_out;
    p.d = d; p.delta = delta; p.partials = partials; p.hd = h; p.h = (float)h; p.ncoef = ncoef; p.stage = stage; p.B = B;
    for (int s = 0; s < VAW_RK_STAGES; ++s) {
        p.ad[s] = s < ncoef ? a[s] : 0.0;
        p.a[s] = (float)p.ad[s];
    }
    const bool vec = vec4_ok(per_sample, model_ld, {out, g, eps, x, x_stage, k, x_out});
    VAW_LAUNCH_W(flow_logp_stage_kernel, vec, grid, 256, stream, p);
    VAW_CHECK_LAUNCH("flow_logp_stage");
    if (grid.x > 1) {
        flow_logp_stage_fold_kernel<<<(B + 255) / 256, 256, 0, (hipStream_t)stream>>>(p, (int)grid.x);
        VAW_CHECK_LAUNCH("flow_logp_stage (fold)");
    }
    return VAW_OK;
}

// log N(z; 0, I) per row = -1/2 sum z^2 - (n/2) ln 2 pi: squares and sum in float64, the order of the stage kernel
template <int W>
__global__ void __launch_bounds__(256) flow_logp_prior_kernel(const float* z, double* logp, double* partials, int64_t n) {
    constexpr bool VEC = W == 4;
    const int64_t base = (int64_t)blockIdx.y * n;
    double acc = 0.0;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; 4 * q < n; q += (int64_t)gridDim.x * blockDim.x) {
        float v[4];
        ldq<VEC>(z + base, 4 * q, n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = acc + (double)v[j] * (double)v[j];
    }
    const double sum = logp_block_sum(acc);
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) logp[blockIdx.y] = -0.5 * sum - 0.5 * (double)n * LN_2PI;
    else partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256) flow_logp_prior_fold_kernel(const double* partials, double* logp, int B, int64_t n, int gx) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sum = partials[(int64_t)b * gx];
    for (int i = 1; i < gx; ++i) sum = sum + partials[(int64_t)b * gx + i];
    logp[b] = -0.5 * sum - 0.5 * (double)n * LN_2PI;
}

extern "C" int vaw_flow_logp_prior(const float* z, double* logp, double* partials, int64_t partials_cap, int B, int64_t per_sample,
                                   vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && per_sample > 0, "flow_logp_prior: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(z && logp, "flow_logp_prior: null pointer");
    VAW_CHECK_ARG(((uintptr_t)logp & 7) == 0 && ((uintptr_t)partials & 7) == 0, "flow_logp_prior: float64 pointer not aligned to 8 bytes");
    const dim3 grid = logp_grid(per_sample, B);
    VAW_CHECK_ARG(grid.x == 1 || (partials && partials_cap >= (int64_t)grid.x * B), "flow_logp_prior: %ld partial sums do not fit %ld",
                  (long)grid.x * B, (long)partials_cap);
    const bool vec = vec4_ok(per_sample, 0, {z});
    VAW_LAUNCH_W(flow_logp_prior_kernel, vec, grid, 256, stream, z, logp, partials, per_sample);
    VAW_CHECK_LAUNCH("flow_logp_prior");
    if (grid.x > 1) {
        flow_logp_prior_fold_kernel<<<(B + 255) / 256, 256, 0, (hipStream_t)stream>>>(partials, logp, B, per_sample, (int)grid.x);
        VAW_CHECK_LAUNCH("flow_logp_prior (fold)");
    }
    return VAW_OK;
}

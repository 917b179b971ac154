// Post-hoc EMA (vaw_amd/ema.py: PowerEMA, posthoc_ema): K <= 4 power-function averages of the flat f32 parameter buffer tracked
// every step, and the f64 fold that turns stored snapshots into the average of any width afterwards.
//
// IEEE arithmetic: every add / multiply below is a separately rounded operation.  The Makefile compiles this file with
// -ffp-contract=off (EXTRA_ema) and the pragma says the same to a build that forgets the flag: the update is then bitwise the f32
// tensor composition e.add((p - e).mul(c)), and the fold bitwise numpy's acc += coef * src.astype(float64).
#include "common.h"

#pragma clang fp contract(off)

static inline bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bbytes && y < x + abytes;
}

// ---- coefficients ----------------------------------------------------------------------------------------------------------------
// One wave.  Every lane reads the counter, the barrier orders those reads before lane 0 writes t back; lane k < K writes c_t of
// profile k.  beta_t = (1 - 1/t)^(gamma+1) = exp((gamma+1) log1p(-1/t)), so c_t = 1 - beta_t = -expm1(...): at t = 1e7 and
// gamma = 7 that is 8e-7, which 1 - pow() would hold to 1e-10 relative and this form holds to the libm's few ulp.
__global__ void __launch_bounds__(64) ema_profiles_coef_kernel(int64_t* __restrict__ step, const double* __restrict__ gamma,
                                                               double* __restrict__ coef, int K) {
    const int64_t t = step[0] + 1;
    __syncthreads();
    if (threadIdx.x == 0) step[0] = t;
    if ((int)threadIdx.x < K)
        coef[threadIdx.x] = t <= 1 ? 1.0 : -expm1((gamma[threadIdx.x] + 1.0) * log1p(-1.0 / (double)t));
}

extern "C" int vaw_ema_profiles_coef(int64_t* step_dev, const double* gamma_dev, double* coef_dev, int K, vaw_stream stream) {
    VAW_CHECK_ARG(K >= 1 && K <= VAW_EMA_MAX_PROFILES, "ema_profiles_coef: K %d is outside 1 .. %d", K, VAW_EMA_MAX_PROFILES);
    VAW_CHECK_ARG(step_dev && gamma_dev && coef_dev, "ema_profiles_coef: step / gamma / coef is NULL");
    ema_profiles_coef_kernel<<<1, 64, 0, (hipStream_t)stream>>>(step_dev, gamma_dev, coef_dev, K);
    VAW_CHECK_LAUNCH("ema_profiles_coef");
    return VAW_OK;
}

// ---- update ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_one(float p, float e, float c) { return c == 1.f ? p : e + (p - e) * c; }

struct EmaBufs {
    float* e[VAW_EMA_MAX_PROFILES];
};

// The tiles and the grid of adamw_ema_kernel (elementwise.hip): a workgroup walks whole tiles of EMA_U x 256 float4 per stream, so a
// lane has EMA_U 16-byte loads of p and of every average in flight before the first use (4 (K + 1) loads, 20 at K = 4 as there);
// every byte is touched once per step and nothing of it is reused before the next one -> non-temporal loads and stores.  The
// partial tile and the n % 4 elements go one group per thread.
#define EMA_U 4
__device__ __forceinline__ f32x4 nt_load4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
template <int K>
__global__ void __launch_bounds__(256) ema_profiles_update_kernel(const float* __restrict__ p, EmaBufs b, int64_t n,
                                                                  const double* __restrict__ coef) {
    float c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = (float)coef[k];
    const int64_t n4 = n / 4;
    constexpr int64_t TILE = (int64_t)EMA_U * 256;                   // float4 per tile
    const int64_t n_tiles = n4 / TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t i0 = t * TILE + threadIdx.x;
        f32x4 pv[EMA_U], ev[K][EMA_U];
#pragma unroll
        for (int u = 0; u < EMA_U; ++u) {
            const int64_t i = 4 * (i0 + 256 * u);
            pv[u] = nt_load4(p + i);
#pragma unroll
            for (int k = 0; k < K; ++k) ev[k][u] = nt_load4(b.e[k] + i);
        }
#pragma unroll
        for (int u = 0; u < EMA_U; ++u) {
            const int64_t i = 4 * (i0 + 256 * u);
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ev[k][u][j] = ema_one(pv[u][j], ev[k][u][j], c[k]);
                __builtin_nontemporal_store(ev[k][u], reinterpret_cast<f32x4*>(b.e[k] + i));
            }
        }
    }
    for (int64_t i = n_tiles * TILE + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 pv = load4(p + 4 * i);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            f32x4 ev = load4(b.e[k] + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) ev[j] = ema_one(pv[j], ev[j], c[k]);
            store4(b.e[k] + 4 * i, ev);
        }
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float pv = p[i];
#pragma unroll
        for (int k = 0; k < K; ++k) b.e[k][i] = ema_one(pv, b.e[k][i], c[k]);
    }
}
static inline int ema_grid(int64_t n) {
    const int64_t tiles = n / 4 / (EMA_U * 256);
    const int64_t cap = 256 * 8;
    return (int)(tiles < 1 ? 1 : (tiles > cap ? cap : tiles));
}

extern "C" int vaw_ema_profiles_update(const float* p, float* e0, float* e1, float* e2, float* e3, int K, int64_t n,
                                       const double* coef_dev, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "ema_profiles_update: n %lld must be positive", (long long)n);
    VAW_CHECK_ARG(K >= 1 && K <= VAW_EMA_MAX_PROFILES, "ema_profiles_update: K %d is outside 1 .. %d", K, VAW_EMA_MAX_PROFILES);
    VAW_CHECK_ARG(p && coef_dev, "ema_profiles_update: p / coef is NULL");
    const void* bufs[VAW_EMA_MAX_PROFILES + 1] = {e0, e1, e2, e3, p};
    bufs[K] = p;                                                      // the K averages, then p: the K + 1 ranges of n floats
    const char* names[VAW_EMA_MAX_PROFILES + 1] = {"e0", "e1", "e2", "e3", "p"};
    names[K] = "p";
    const size_t bytes = (size_t)n * sizeof(float);
    for (int k = 0; k <= K; ++k) {
        VAW_CHECK_ARG(bufs[k], "ema_profiles_update: %s is NULL (K = %d)", names[k], K);
        VAW_CHECK_ARG(al16(bufs[k]), "ema_profiles_update: %s is not 16-byte aligned", names[k]);
        for (int j = 0; j < k; ++j)
            VAW_CHECK_ARG(!ranges_overlap(bufs[j], bytes, bufs[k], bytes), "ema_profiles_update: %s overlaps %s", names[j], names[k]);
    }
    EmaBufs b{{e0, e1, e2, e3}};
    const dim3 grid(ema_grid(n));
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
        case 1: ema_profiles_update_kernel<1><<<grid, 256, 0, s>>>(p, b, n, coef_dev); break;
        case 2: ema_profiles_update_kernel<2><<<grid, 256, 0, s>>>(p, b, n, coef_dev); break;
        case 3: ema_profiles_update_kernel<3><<<grid, 256, 0, s>>>(p, b, n, coef_dev); break;
        default: ema_profiles_update_kernel<4><<<grid, 256, 0, s>>>(p, b, n, coef_dev); break;
    }
    VAW_CHECK_LAUNCH("ema_profiles_update");
    return VAW_OK;
}

// ---- reconstruction --------------------------------------------------------------------------------------------------------------
// Two plain streams (12 B and 12 B per element), four elements per thread and pass where the pointers allow 16-byte accesses.
template <int W>
__global__ void __launch_bounds__(256) lincomb_accum_f64_kernel(double* __restrict__ acc, const float* __restrict__ src, double coef,
                                                                int64_t n) {
    const int64_t items = W == 4 ? n / 4 : n;
    for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        float s[W];
        double a[W];
        loadw<W>(src + W * it, s);
        loadw<W>(acc + W * it, a);
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = a[j] + coef * (double)s[j];
        storew<W>(acc + W * it, a);
    }
    if (W == 4)
        for (int64_t i = items * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            acc[i] = acc[i] + coef * (double)src[i];
}
template <int W>
__global__ void __launch_bounds__(256) f64_to_f32_kernel(const double* __restrict__ acc, float* __restrict__ out, int64_t n) {
    const int64_t items = W == 4 ? n / 4 : n;
    for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        double a[W];
        float o[W];
        loadw<W>(acc + W * it, a);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = (float)a[j];
        storew<W>(out + W * it, o);
    }
    if (W == 4)
        for (int64_t i = items * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            out[i] = (float)acc[i];
}
static inline int fold_grid(int64_t items) {
    const int64_t g = (items + 255) / 256, cap = 256 * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" int vaw_lincomb_accum_f64(double* acc, const float* src, double coef, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "lincomb_accum_f64: n %lld must be positive", (long long)n);
    VAW_CHECK_ARG(acc && src, "lincomb_accum_f64: acc / src is NULL");
    VAW_CHECK_ARG(!ranges_overlap(acc, (size_t)n * 8, src, (size_t)n * 4), "lincomb_accum_f64: acc and src overlap");
    const bool vec = al16(acc) && al16(src);
    VAW_LAUNCH_W(lincomb_accum_f64_kernel, vec, fold_grid(vec ? n / 4 + 1 : n), 256, stream, acc, src, coef, n);
    VAW_CHECK_LAUNCH("lincomb_accum_f64");
    return VAW_OK;
}

extern "C" int vaw_f64_to_f32(const double* acc, float* out, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0, "f64_to_f32: n %lld must be positive", (long long)n);
    VAW_CHECK_ARG(acc && out, "f64_to_f32: acc / out is NULL");
    VAW_CHECK_ARG(!ranges_overlap(acc, (size_t)n * 8, out, (size_t)n * 4), "f64_to_f32: acc and out overlap");
    const bool vec = al16(acc) && al16(out);
    VAW_LAUNCH_W(f64_to_f32_kernel, vec, fold_grid(vec ? n / 4 + 1 : n), 256, stream, acc, out, n);
    VAW_CHECK_LAUNCH("f64_to_f32");
    return VAW_OK;
}

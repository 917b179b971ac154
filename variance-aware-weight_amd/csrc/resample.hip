// Device-resident loss-second-moment timestep sampler (vaw_amd/resample.py: DeviceLossSecondMomentResampler): the [T][H] f64 loss
// history and the [T] counters of LossSecondMomentResampler live in HBM; one launch records a batch of (t, loss) pairs, one
// launch turns the history into p, its CDF and a batch of draws.  No atomics on the history: a timestep has one owner thread.
//
// IEEE arithmetic: every f64 add / multiply / divide / sqrt below is a separately rounded operation.  The Makefile compiles this
// file with -ffp-contract=off (EXTRA_resample) and the pragma below says the same to a build that forgets the flag, so the square
// is never fused into the sum of squares; no fast-math flag is on the command line, and f64 '/' and sqrt() are correctly rounded
// in device code (the f32-only relaxations of hipcc do not touch them).
#include "common.h"

#pragma clang fp contract(off)

#define RS_UPD_THREADS 64        // one wave per workgroup: thread = timestep
#define RS_UPD_CHUNK 1024        // (t, loss) pairs staged in LDS at a time (8 KiB)
#define RS_DRAW_THREADS 512

// ---- update --------------------------------------------------------------------------------------------------------------------
// Thread `me` owns timestep `me`: it walks the whole batch in order (staged through LDS in chunks, every lane reads the same
// word: a broadcast) and appends the losses whose t is its own.  Nothing depends on the grid or block size.  Entries outside
// [0, T) are staged as t = -1, which no thread owns; workgroup 0 counts them and its thread 0 adds the count to bad[0].
// FINITE_ONLY (vaw_resampler_update_finite, the step guard's form): a pair whose loss is inf or NaN is staged and counted the same
// way, so a poisoned step never enters the history the draws are formed from.
template <bool FINITE_ONLY>
__global__ void __launch_bounds__(RS_UPD_THREADS) resampler_update_kernel(const int64_t* __restrict__ ts, const float* __restrict__ losses,
                                                                          int n, int T, int H, double* __restrict__ ring,
                                                                          int64_t* __restrict__ seen, int* __restrict__ bad) {
    __shared__ int2 stage[RS_UPD_CHUNK];          // {t or -1, loss bits}
    const int me = blockIdx.x * RS_UPD_THREADS + threadIdx.x;
    const bool own = me < T;
    int64_t cnt = own ? seen[me] : 0;
    int slot = own ? (int)(((cnt % H) + H) % H) : 0;          // (a negative counter cannot index outside the row)
    double* row = ring + (size_t)(own ? me : 0) * H;
    int nbad = 0;
    for (int c0 = 0; c0 < n; c0 += RS_UPD_CHUNK) {
        const int m = min(RS_UPD_CHUNK, n - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += RS_UPD_THREADS) {
            const int64_t t = ts[c0 + i];
            const int bits = __float_as_int(losses[c0 + i]);
            const bool ok = t >= 0 && t < T && (!FINITE_ONLY || (bits & 0x7f800000) != 0x7f800000);
            nbad += ok ? 0 : 1;
            stage[i] = make_int2(ok ? (int)t : -1, bits);
        }
        __syncthreads();
        if (own) {
#pragma unroll 8
            for (int i = 0; i < m; ++i) {
                const int2 e = stage[i];
                if (e.x == me) {
                    row[slot] = (double)__int_as_float(e.y);
                    slot = slot + 1 == H ? 0 : slot + 1;
                    ++cnt;
                }
            }
        }
    }
    if (own) seen[me] = cnt;
    if (blockIdx.x == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
        if (threadIdx.x == 0 && nbad) bad[0] += nbad;          // the only writer of bad[] in this launch
    }
}

static int resampler_update_launch(const char* what, bool finite_only, const int64_t* ts, const float* losses, int n, int T, int H,
                                   double* ring, int64_t* seen, int* bad, vaw_stream stream) {
    VAW_CHECK_ARG(T > 0 && H > 0 && n >= 0, "%s: T %d and H %d must be positive, n %d not negative", what, T, H, n);
    VAW_CHECK_ARG(ring && seen && bad, "%s: ring / seen / bad is NULL", what);
    if (n == 0) return VAW_OK;
    VAW_CHECK_ARG(ts && losses, "%s: ts / losses is NULL", what);
    const int grid = ceil_div(T, RS_UPD_THREADS);
    if (finite_only) resampler_update_kernel<true><<<grid, RS_UPD_THREADS, 0, (hipStream_t)stream>>>(ts, losses, n, T, H, ring, seen, bad);
    else resampler_update_kernel<false><<<grid, RS_UPD_THREADS, 0, (hipStream_t)stream>>>(ts, losses, n, T, H, ring, seen, bad);
    VAW_CHECK_LAUNCH(what);
    return VAW_OK;
}
extern "C" int vaw_resampler_update(const int64_t* ts, const float* losses, int n, int T, int H, double* ring, int64_t* seen,
                                    int* bad, vaw_stream stream) {
    return resampler_update_launch("resampler_update", false, ts, losses, n, T, H, ring, seen, bad, stream);
}
extern "C" int vaw_resampler_update_finite(const int64_t* ts, const float* losses, int n, int T, int H, double* ring, int64_t* seen,
                                           int* bad, vaw_stream stream) {
    return resampler_update_launch("resampler_update_finite", true, ts, losses, n, T, H, ring, seen, bad, stream);
}

// ---- draw ----------------------------------------------------------------------------------------------------------------------
// One workgroup; LDS holds pw[T] (w, then p in place) and cdf[T], 16 T bytes: T <= VAW_RESAMPLER_MAX_T fills the 64 KiB a launch
// may ask for without raising its cap.  Orders of summation (also in include/vaw_hip.h):
//   mean of squares of a timestep: j = 0 .. H-1 ascending, one accumulator, then one division by H;
//   sum of w: 64 partial sums, partial l = w[l] + w[l+64] + w[l+128] + ... ascending, then the partials l = 0 .. 63 ascending;
//   cdf: strictly left to right, one accumulator, then every entry divided by the last.
__global__ void __launch_bounds__(RS_DRAW_THREADS) resampler_draw_kernel(const double* __restrict__ ring, const int64_t* __restrict__ seen,
                                                                         int T, int H, double uniform_prob, const double* __restrict__ u,
                                                                         int B, int64_t* __restrict__ out_t, float* __restrict__ out_w,
                                                                         double* __restrict__ p_out) {
    extern __shared__ double rs_lds[];
    double* pw = rs_lds;
    double* cdf = rs_lds + T;
    int* flag = reinterpret_cast<int*>(cdf);           // cdf is scratch until the running sum is formed
    const int tid = threadIdx.x;

    if (tid == 0) flag[0] = 1;
    __syncthreads();
    bool cold = false;
    for (int t = tid; t < T; t += RS_DRAW_THREADS) cold |= seen[t] < (int64_t)H;
    if (cold) flag[0] = 0;                             // (every writer stores the same value)
    __syncthreads();
    const bool warm = flag[0] != 0;
    __syncthreads();

    if (!warm) {
        const double pu = 1.0 / (double)T;
        for (int t = tid; t < T; t += RS_DRAW_THREADS) pw[t] = pu;
    } else {
        for (int t = tid; t < T; t += RS_DRAW_THREADS) {
            const double* row = ring + (size_t)t * H;
            double s = 0.0;
            for (int j = 0; j < H; ++j) {
                const double v = row[j];
                s = s + v * v;
            }
            pw[t] = sqrt(s / (double)H);
        }
        __syncthreads();
        if (tid < 64) {                                // wave 0: lane l holds partial l, every lane folds them in lane order
            double s = 0.0;
            for (int t = tid; t < T; t += 64) s = s + pw[t];
            double S = 0.0;
            for (int l = 0; l < 64; ++l) S = S + __shfl(s, l, 64);
            if (tid == 0) cdf[0] = S;
        }
        __syncthreads();
        const double S = cdf[0];
        __syncthreads();
        const double keep = 1.0 - uniform_prob, floor_p = uniform_prob / (double)T;
        for (int t = tid; t < T; t += RS_DRAW_THREADS) pw[t] = pw[t] / S * keep + floor_p;
    }
    __syncthreads();
    for (int t = tid; t < T; t += RS_DRAW_THREADS) p_out[t] = pw[t];

    if (tid == 0) {
        // loads of a batch first, then the dependent adds: the compiler may not move an LDS load above the store before it
        double s = 0.0;
        for (int t0 = 0; t0 < T; t0 += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = t0 + k < T ? pw[t0 + k] : 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (t0 + k < T) {
                    s = s + v[k];
                    cdf[t0 + k] = s;
                }
        }
    }
    __syncthreads();
    const double total = cdf[T - 1];
    __syncthreads();
    for (int t = tid; t < T; t += RS_DRAW_THREADS) cdf[t] = cdf[t] / total;
    __syncthreads();

    for (int b = tid; b < B; b += RS_DRAW_THREADS) {
        const double x = u[b];
        int lo = 0, hi = T;                            // number of cdf entries <= x (searchsorted, side = "right")
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        lo = min(lo, T - 1);                           // x >= 1 (not a uniform of [0, 1)) must not index past the tables
        out_t[b] = lo;
        out_w[b] = (float)(1.0 / ((double)T * pw[lo]));
    }
}

extern "C" int vaw_resampler_draw(const double* ring, const int64_t* seen, int T, int H, double uniform_prob, const double* u, int B,
                                  int64_t* out_t, float* out_w, double* p, vaw_stream stream) {
    VAW_CHECK_ARG(T > 0 && H > 0 && B >= 0, "resampler_draw: T %d and H %d must be positive, B %d not negative", T, H, B);
    VAW_CHECK_ARG(T <= VAW_RESAMPLER_MAX_T, "resampler_draw: T %d is more than the %d timesteps one workgroup's LDS holds (16 bytes each)",
                  T, VAW_RESAMPLER_MAX_T);
    VAW_CHECK_ARG(uniform_prob >= 0.0 && uniform_prob <= 1.0, "resampler_draw: uniform_prob %g is not in [0, 1]", uniform_prob);
    VAW_CHECK_ARG(ring && seen && p, "resampler_draw: ring / seen / p is NULL");
    VAW_CHECK_ARG(B == 0 || (u && out_t && out_w), "resampler_draw: u / out_t / out_w is NULL");
    resampler_draw_kernel<<<1, RS_DRAW_THREADS, (size_t)T * 16, (hipStream_t)stream>>>(ring, seen, T, H, uniform_prob, u, B, out_t, out_w, p);
    VAW_CHECK_LAUNCH("resampler_draw");
    return VAW_OK;
}

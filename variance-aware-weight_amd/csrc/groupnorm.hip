// GroupNorm32 (+ FiLM scale/shift, + SiLU) forward / backward on NHWC activations [B, HW, C]     tools/nn.py:17-19,93-100,
// unet.py:236-256: the channel-quad kernels, the flat 16-byte bf16 kernels, vaw_gn_plan -- the one place that chooses between
// them -- and the three entry points.  All HBM-bound; reductions in a fixed order (no float atomics).
#include "common.h"

#include <type_traits>

#define BY_DTYPE(dt, CALL)                      \
    if (dt == VAW_F32) { using T = float; CALL; } \
    else { using T = bf16_t; CALL; }

// ---------------------------------------------------------------------------------------------
// GroupNorm32 (+FiLM, +SiLU) forward and backward as streaming passes over [B, HW, C].  Every pass uses one
// thread mapping: a block covers 64 channels x one chunk of 512 pixels of one sample; a thread owns a channel QUAD
// (8-byte bf16 / 16-byte f32 accesses) and one of 16 row groups, so all per-channel parameters (mean, rstd, gamma,
// beta, FiLM scale/shift, group sums) are loaded once per thread and the row loop is pure streaming.
//   sums    per-(sample, channel) partial sums per chunk -> tiny group kernel folds chunks and channels in a fixed
//           order (double accumulation for the variance)
//   apply   y = act(GN(x)*gamma+beta [*(1+scale)+shift])    /    dx = rstd*(dn1*gamma - S1/N - xhat*S2/N) (+ dx_add)
// ---------------------------------------------------------------------------------------------
#define GN_ROWS 512
// SiLU and its derivative through v_rcp_f32 (1 ulp) instead of an IEEE division (~10 more instructions per element): the
// GroupNorm passes are close enough to VALU-bound at 4 waves per SIMD for that to show
__device__ __forceinline__ float gn_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float gn_silu(float x) { return x * gn_sigmoid(x); }
__device__ __forceinline__ float gn_silu_grad(float x) {
    const float s = gn_sigmoid(x);
    return s * (1.f + x * (1.f - s));
}

struct GnQuad {   // per-thread constants for its 4 channels
    f32x4 mu, rs, ga, be, sc, sh;
};
__device__ __forceinline__ GnQuad gn_quad(const float* mean, const float* rstd, const float* gamma, const float* beta,
                                          const float* scale, const float* shift, int64_t film_ld, int b, int c, int C, int G) {
    GnQuad q;
    const int cg = C / G;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = (c + j) / cg;
        q.mu[j] = mean[b * G + g];
        q.rs[j] = rstd[b * G + g];
    }
    q.ga = load4(gamma + c);
    q.be = load4(beta + c);
    q.sc = scale ? load4(scale + (int64_t)b * film_ld + c) : f32x4{0, 0, 0, 0};
    q.sh = scale ? load4(shift + (int64_t)b * film_ld + c) : f32x4{0, 0, 0, 0};
    return q;
}

template <typename T>
__global__ void __launch_bounds__(256)
gn_fwd_sums_kernel(const T* __restrict__ x, int HW, int C, int B, int nchunk, float* __restrict__ part /* [2][nchunk][B][C] */) {
    __shared__ __attribute__((aligned(16))) float red[2][16][64];
    const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4, b = blockIdx.y, chunk = blockIdx.z;
    f32x4 s = {0, 0, 0, 0}, q = {0, 0, 0, 0};
    if (c < C) {
        const int r0 = chunk * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
        const T* p = x + (int64_t)b * HW * C + c;
        for (int r = r0 + rg; r < r1; r += 16) {
            const f32x4 v = load4(p + (int64_t)r * C);
            s += v;
            q += v * v;
        }
    }
    store4(&red[0][rg][cq * 4], s);
    store4(&red[1][rg][cq * 4], q);
    __syncthreads();
    const int cl = threadIdx.x & 63, k = threadIdx.x >> 6;
    if (k < 2 && blockIdx.x * 64 + cl < C) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[k][g][cl];
        part[(((int64_t)k * nchunk + chunk) * B + b) * C + blockIdx.x * 64 + cl] = t;
    }
}

__global__ void gn_group_stats_kernel(const float* __restrict__ part, int nchunk, int B, int C, int G, int HW, float eps,
                                      float* __restrict__ mean, float* __restrict__ rstd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * G) return;
    const int b = i / G, g = i % G, cg = C / G;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < nchunk; ++ch)
        for (int j = 0; j < cg; ++j) {
            s += (double)part[(((int64_t)0 * nchunk + ch) * B + b) * C + g * cg + j];
            q += (double)part[(((int64_t)1 * nchunk + ch) * B + b) * C + g * cg + j];
        }
    const double n = (double)cg * HW;
    const double m = s / n;
    double var = q / n - m * m;
    if (var < 0.0) var = 0.0;
    mean[i] = (float)m;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

template <typename T>
__global__ void __launch_bounds__(256)
gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ scale,
                const float* __restrict__ shift, int64_t film_ld, int silu, T* __restrict__ y, int HW, int C, int G) {
    const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4, b = blockIdx.y, chunk = blockIdx.z;
    if (c >= C) return;
    const GnQuad k = gn_quad(mean, rstd, gamma, beta, scale, shift, film_ld, b, c, C, G);
    const f32x4 a1 = k.rs * k.ga, b1 = k.be - k.mu * k.rs * k.ga;       // n1 = x*a1 + b1
    const int r0 = chunk * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
    const int64_t base = (int64_t)b * HW * C + c;
    for (int r = r0 + rg; r < r1; r += 16) {
        f32x4 n = load4(x + base + (int64_t)r * C) * a1 + b1;
        if (scale) n = n * (1.f + k.sc) + k.sh;
        if (silu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) n[j] = gn_silu(n[j]);
        }
        store4(y + base + (int64_t)r * C, n);
    }
}

// Backward sums per (sample, channel): A = dn1*xhat, Bs = dn1, DS = dn2*n1, DH = dn2
//   (n1 = xhat*gamma+beta, n2 = FiLM(n1), dn2 = dout*act'(n2), dn1 = dn2*(1+scale))
template <typename T>
__global__ void __launch_bounds__(256)
gn_bwd_sums_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ mean,
                   const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                   const float* __restrict__ scale, const float* __restrict__ shift, int64_t film_ld, int silu, int HW, int C,
                   int G, int B, int nchunk, float* __restrict__ part /* [4][nchunk][B][C] */) {
    __shared__ __attribute__((aligned(16))) float red[4][16][64];
    const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4, b = blockIdx.y, chunk = blockIdx.z;
    f32x4 a = {0, 0, 0, 0}, bs = {0, 0, 0, 0}, ds = {0, 0, 0, 0}, dh = {0, 0, 0, 0};
    if (c < C) {
        const GnQuad k = gn_quad(mean, rstd, gamma, beta, scale, shift, film_ld, b, c, C, G);
        const int r0 = chunk * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
        const int64_t base = (int64_t)b * HW * C + c;
        for (int r = r0 + rg; r < r1; r += 16) {
            const f32x4 xh = (load4(x + base + (int64_t)r * C) - k.mu) * k.rs;
            const f32x4 n1 = xh * k.ga + k.be;
            const f32x4 n2 = scale ? n1 * (1.f + k.sc) + k.sh : n1;
            f32x4 dn2 = load4(dout + base + (int64_t)r * C);
            if (silu) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dn2[j] *= gn_silu_grad(n2[j]);
            }
            const f32x4 dn1 = scale ? dn2 * (1.f + k.sc) : dn2;
            a += dn1 * xh;
            bs += dn1;
            ds += dn2 * n1;
            dh += dn2;
        }
    }
    store4(&red[0][rg][cq * 4], a);
    store4(&red[1][rg][cq * 4], bs);
    store4(&red[2][rg][cq * 4], ds);
    store4(&red[3][rg][cq * 4], dh);
    __syncthreads();
    const int cl = threadIdx.x & 63, kk = threadIdx.x >> 6;
    if (blockIdx.x * 64 + cl < C) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[kk][g][cl];
        part[(((int64_t)kk * nchunk + chunk) * B + b) * C + blockIdx.x * 64 + cl] = t;
    }
}

// fold chunks -> per (b,c) sums; per (b,g): S1 = sum_c gamma_c*Bs, S2 = sum_c gamma_c*A; dgamma/dbeta over samples;
// FiLM gradients into the rows of the emb_layers output gradient.  One thread per (b, c) for the folds (fixed order).
__global__ void gn_bwd_fold_kernel(const float* __restrict__ part, int nchunk, int B, int C, float* __restrict__ sums /* [4][B][C] */) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)4 * B * C) return;
    const int64_t k = i / ((int64_t)B * C), bc = i % ((int64_t)B * C);
    float t = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) t += part[((k * nchunk + ch) * B) * C + bc];
    sums[i] = t;
}
// Three independent jobs in one launch, told apart by block index (each fully parallel; fixed summation order):
//   blocks [0, nb1)        S1, S2 per (sample, group)
//   blocks [nb1, nb1+nb2)  dgamma, dbeta: 16 channels per block, 16 lanes stride the batch, shuffle tree over them
//   blocks [nb1+nb2, ...)  FiLM gradients copied out per (sample, channel)
// `sums` is gn_bwd_fold_kernel's [4][B][C] (folding the chunks in here saves that launch and was measured SLOWER: 15.6 us against 5.4 + 4.9)
__global__ void __launch_bounds__(256)
gn_bwd_group_kernel(const float* __restrict__ sums, const float* __restrict__ gamma, int B, int C, int G,
                    float* __restrict__ S1, float* __restrict__ S2, float* __restrict__ dgamma,
                    float* __restrict__ dbeta, float gbeta, float* __restrict__ dscale,
                    float* __restrict__ dshift, int64_t dfilm_ld, int nb1, int nb2) {
    const int cg = C / G;
    const int64_t BC = (int64_t)B * C;
    int blk = blockIdx.x;
    if (blk < nb1) {
        const int i = blk * 256 + threadIdx.x;
        if (i >= B * G) return;
        const int b = i / G, g = i % G;
        float s1 = 0.f, s2 = 0.f;
        for (int j = 0; j < cg; ++j) {
            const int c = g * cg + j;
            s1 += gamma[c] * sums[BC + (int64_t)b * C + c];
            s2 += gamma[c] * sums[(int64_t)b * C + c];
        }
        S1[i] = s1;
        S2[i] = s2;
        return;
    }
    blk -= nb1;
    if (blk < nb2) {
        const int c = blk * 16 + (threadIdx.x & 15), bl = threadIdx.x >> 4;     // 16 channels x 16 batch lanes
        float dg = 0.f, db = 0.f;
        if (c < C)
            for (int b = bl; b < B; b += 16) {
                dg += sums[(int64_t)b * C + c];
                db += sums[BC + (int64_t)b * C + c];
            }
        // lanes of one channel sit 16 apart: in-wave tree over lane bits 4,5, then the 4 waves through LDS
        dg += __shfl_xor(dg, 16, 64); dg += __shfl_xor(dg, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        __shared__ float red[2][4][16];
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane < 16) { red[0][w][lane] = dg; red[1][w][lane] = db; }
        __syncthreads();
        if (threadIdx.x < 16 && c < C) {
            const float tg = (red[0][0][threadIdx.x] + red[0][1][threadIdx.x]) + (red[0][2][threadIdx.x] + red[0][3][threadIdx.x]);
            const float tb = (red[1][0][threadIdx.x] + red[1][1][threadIdx.x]) + (red[1][2][threadIdx.x] + red[1][3][threadIdx.x]);
            dgamma[c] = (gbeta != 0.f ? gbeta * dgamma[c] : 0.f) + tg;
            dbeta[c] = (gbeta != 0.f ? gbeta * dbeta[c] : 0.f) + tb;
        }
        return;
    }
    blk -= nb2;
    const int64_t i = (int64_t)blk * 256 + threadIdx.x;
    if (dscale && i < BC) {
        const int64_t b = i / C, c = i % C;
        dscale[b * dfilm_ld + c] = sums[2 * BC + i];
        dshift[b * dfilm_ld + c] = sums[3 * BC + i];
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
gn_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ mean,
                    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const float* __restrict__ scale, const float* __restrict__ shift, int64_t film_ld, int silu,
                    const float* __restrict__ S1, const float* __restrict__ S2, const T* __restrict__ dx_add,
                    T* __restrict__ dx, int HW, int C, int G) {
    const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4, b = blockIdx.y, chunk = blockIdx.z;
    if (c >= C) return;
    const GnQuad k = gn_quad(mean, rstd, gamma, beta, scale, shift, film_ld, b, c, C, G);
    const int cg = C / G;
    const float invn = 1.f / ((float)cg * HW);
    f32x4 t1, t2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = (c + j) / cg;
        t1[j] = S1[b * G + g] * invn;
        t2[j] = S2[b * G + g] * invn;
    }
    const int r0 = chunk * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
    const int64_t base = (int64_t)b * HW * C + c;
    for (int r = r0 + rg; r < r1; r += 16) {
        const int64_t e = base + (int64_t)r * C;
        const f32x4 xh = (load4(x + e) - k.mu) * k.rs;
        const f32x4 n1 = xh * k.ga + k.be;
        const f32x4 n2 = scale ? n1 * (1.f + k.sc) + k.sh : n1;
        f32x4 dn2 = load4(dout + e);
        if (silu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) dn2[j] *= gn_silu_grad(n2[j]);
        }
        const f32x4 dn1 = scale ? dn2 * (1.f + k.sc) : dn2;
        f32x4 r4 = k.rs * (dn1 * k.ga - t1 - xh * t2);
        if (dx_add) r4 += load4(dx_add + e);
        store4(dx + e, r4);
    }
}

// ---------------------------------------------------------------------------------------------
// The same four passes for bf16 with C % 8 == 0 on a FLAT mapping (the recipe that took the AdamW and row kernels from
// 4-5 to 5-6.5 TB/s): a thread owns one channel OCTET (16-byte accesses) and every rpi-th row, nt = a multiple of C/8 lanes
// are live, so one step of a workgroup is nt x 16 CONTIGUOUS bytes; U steps are in flight per lane and stream before the
// first is consumed; non-temporal accesses for everything that is not read again soon (the forward sums pass leaves x in
// the caches for the apply pass, which walks the chunks in the opposite order so that it starts on the freshest ones).
// Chunks (GN_ROWS rows), workspace layouts and the small fold / group kernels are those of the quad-mapped kernels above,
// which stay for everything vaw_gn_plan does not give to these.  Backward sums: with d = dout act'(n2) only sd = sum d and
// sx = sum d (x - mu) are accumulated; A, Bs, DS, DH are formed from them when the chunk's sums are written.
// ---------------------------------------------------------------------------------------------
#define GNS_NT 256
struct GnsGeom {
    int C8, nt, rpi, rows;     // rows per chunk
};
__device__ __forceinline__ void gns_st_nt(bf16_t* p, const float (&f)[8]) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16_t)f[j];
    __builtin_nontemporal_store(v, reinterpret_cast<bf16x8*>(p));
}
// per-thread sums of 8 channels x 2 quantities -> per-channel sums of the chunk in chs[2][C] (C <= 2048)
__device__ __forceinline__ void gns_fold(const float (&s)[8], const float (&q)[8], float* red, float* chs, int C, int rpi, int rl, int c0,
                                         bool live) {
    if (live) {
        float* w0 = red + rl * C + c0;
        float* w1 = red + (rpi + rl) * C + c0;
        *reinterpret_cast<f32x4*>(w0) = f32x4{s[0], s[1], s[2], s[3]};
        *reinterpret_cast<f32x4*>(w0 + 4) = f32x4{s[4], s[5], s[6], s[7]};
        *reinterpret_cast<f32x4*>(w1) = f32x4{q[0], q[1], q[2], q[3]};
        *reinterpret_cast<f32x4*>(w1 + 4) = f32x4{q[4], q[5], q[6], q[7]};
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * C; c += GNS_NT) {
        const int k = c >= C ? 1 : 0, cc = c - k * C;
        const float* p = red + k * rpi * C + cc;
        float t = 0.f;
        for (int r = 0; r < rpi; ++r) t += p[r * C];
        chs[c] = t;
    }
    __syncthreads();
}

// Per-channel coefficients of a thread's octet, shared by the apply and both backward kernels:  n2 = x P + Q,
// P = rstd gamma (1+scale),  Q = (beta - mu rstd gamma)(1+scale) + shift  ((x a + b)(1 + scale) + shift as one multiply-add);
// mu / rs: the statistics of each channel's group
template <bool FILM>
__device__ __forceinline__ void gns_coef(const float* mean, const float* rstd, const float* gamma, const float* beta, const float* scale,
                                         const float* shift, int64_t film_ld, int b, int c0, int cg, int G, float (&P)[8], float (&Q)[8],
                                         float (&mu)[8], float (&rs)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int g = (c0 + j) / cg;
        mu[j] = mean[b * G + g];
        rs[j] = rstd[b * G + g];
        const float ga = gamma[c0 + j];
        P[j] = rs[j] * ga;
        Q[j] = beta[c0 + j] - mu[j] * rs[j] * ga;
        if (FILM) {
            const float s1 = 1.f + scale[(int64_t)b * film_ld + c0 + j];
            P[j] *= s1;
            Q[j] = Q[j] * s1 + shift[(int64_t)b * film_ld + c0 + j];
        }
    }
}

template <int U>
__global__ void __launch_bounds__(GNS_NT)
gns_fwd_sums_kernel(const bf16_t* __restrict__ x, int HW, int C, int B, int nchunk, GnsGeom gm, float* __restrict__ part /* [2][nchunk][B][C] */) {
    __shared__ __attribute__((aligned(16))) float red[2 * GNS_NT * 8];
    __shared__ float chs[2 * 2048];
    const int t = threadIdx.x, b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
    const bool live = t < gm.nt;
    const int oct = live ? t % gm.C8 : 0, rl = live ? t / gm.C8 : 0, c0 = oct * 8;
    const int r0 = chunk * gm.rows, r1 = r0 + gm.rows < HW ? r0 + gm.rows : HW;
    const bf16_t* xs = x + (int64_t)b * HW * C;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
    for (int rb = r0 + rl; rb < r1; rb += U * gm.rpi) {
        gns_u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r = rb + u * gm.rpi;
            r = r < r1 ? r : r1 - 1;
            v[u] = gns_ld(xs + (unsigned)(r * C + c0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = live && rb + u * gm.rpi < r1;
            float f[8];
            gns_unpack(v[u], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float a = ok ? f[j] : 0.f;
                s[j] += a;
                q[j] += a * a;
            }
        }
    }
    gns_fold(s, q, red, chs, C, gm.rpi, rl, c0, live);
    for (int c = t; c < 2 * C; c += GNS_NT) {
        const int k = c >= C ? 1 : 0, cc = c - k * C;
        part[(((int64_t)k * nchunk + chunk) * B + b) * C + cc] = chs[c];
    }
}

template <int U, bool SILU, bool FILM>
__global__ void __launch_bounds__(GNS_NT)
gns_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                 const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ scale,
                 const float* __restrict__ shift, int64_t film_ld, bf16_t* __restrict__ y, int HW, int C, int G, int nchunk, GnsGeom gm) {
    const int item = gridDim.x - 1 - blockIdx.x;             // the sums pass went 0 .. n-1: start on what it read last
    const int t = threadIdx.x, b = item / nchunk, chunk = item - b * nchunk;
    if (t >= gm.nt) return;
    const int oct = t % gm.C8, rl = t / gm.C8, c0 = oct * 8, cg = C / G;
    const int r0 = chunk * gm.rows, r1 = r0 + gm.rows < HW ? r0 + gm.rows : HW;
    const bf16_t* xs = x + (int64_t)b * HW * C;
    bf16_t* ys = y + (int64_t)b * HW * C;
    float a1[8], b1[8], mu[8], rs[8];
    gns_coef<FILM>(mean, rstd, gamma, beta, scale, shift, film_ld, b, c0, cg, G, a1, b1, mu, rs);
    for (int rb = r0 + rl; rb < r1; rb += U * gm.rpi) {
        gns_u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r = rb + u * gm.rpi;
            r = r < r1 ? r : r1 - 1;
            v[u] = gns_ld_nt(xs + (unsigned)(r * C + c0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = rb + u * gm.rpi;
            float f[8], o[8];
            gns_unpack(v[u], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float n = f[j] * a1[j] + b1[j];
                if (SILU) n = gn_silu(n);
                o[j] = n;
            }
            if (r < r1) gns_st_nt(ys + (unsigned)(r * C + c0), o);
        }
    }
}

template <int U, bool SILU, bool FILM>
__global__ void __launch_bounds__(GNS_NT)
gns_bwd_sums_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ x, const float* __restrict__ mean,
                    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const float* __restrict__ scale, const float* __restrict__ shift, int64_t film_ld, int HW, int C, int G, int B,
                    int nchunk, GnsGeom gm, float* __restrict__ part /* [4][nchunk][B][C] */) {
    __shared__ __attribute__((aligned(16))) float red[2 * GNS_NT * 8];
    __shared__ float chs[2 * 2048];
    const int t = threadIdx.x, b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
    const bool live = t < gm.nt;
    const int oct = live ? t % gm.C8 : 0, rl = live ? t / gm.C8 : 0, c0 = oct * 8, cg = C / G;
    const int r0 = chunk * gm.rows, r1 = r0 + gm.rows < HW ? r0 + gm.rows : HW;
    const bf16_t *xs = x + (int64_t)b * HW * C, *ds = dout + (int64_t)b * HW * C;
    float P[8], Q[8], mu[8], rs8[8];
    gns_coef<FILM>(mean, rstd, gamma, beta, scale, shift, film_ld, b, c0, cg, G, P, Q, mu, rs8);
    float sd[8], sx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sd[j] = sx[j] = 0.f;
    for (int rb = r0 + rl; rb < r1; rb += U * gm.rpi) {
        gns_u32x4 xv[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r = rb + u * gm.rpi;
            r = r < r1 ? r : r1 - 1;
            xv[u] = gns_ld(xs + (unsigned)(r * C + c0));
            dv[u] = gns_ld(ds + (unsigned)(r * C + c0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = live && rb + u * gm.rpi < r1;
            float xf[8], df[8];
            gns_unpack(xv[u], xf);
            gns_unpack(dv[u], df);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = df[j];
                if (SILU) d *= gn_silu_grad(xf[j] * P[j] + Q[j]);
                d = ok ? d : 0.f;
                sd[j] += d;
                sx[j] += d * (xf[j] - mu[j]);
            }
        }
    }
    gns_fold(sd, sx, red, chs, C, gm.rpi, rl, c0, live);
    // A = (1+scale) rstd sx,  Bs = (1+scale) sd,  DS = gamma rstd sx + beta sd,  DH = sd
    const int64_t plane = (int64_t)nchunk * B * C;
    for (int c = t; c < C; c += GNS_NT) {
        const float d0 = chs[c], x0 = chs[C + c];
        const float rs = rstd[b * G + c / cg];
        const float s1 = FILM ? 1.f + scale[(int64_t)b * film_ld + c] : 1.f;
        float* o = part + ((int64_t)chunk * B + b) * C + c;
        o[0] = s1 * (rs * x0);
        o[plane] = s1 * d0;
        o[2 * plane] = gamma[c] * (rs * x0) + beta[c] * d0;
        o[3 * plane] = d0;
    }
}

// dx = rstd (dn1 gamma - S1/N - xhat S2/N) + dx_add  =  P d - K3 x - K2 (+ dx_add),  K3 = rstd^2 S2/N,  K2 = rstd S1/N - K3 mu
template <int U, bool SILU, bool FILM, bool ADD>
__global__ void __launch_bounds__(GNS_NT)
gns_bwd_apply_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ x, const float* __restrict__ mean,
                     const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                     const float* __restrict__ scale, const float* __restrict__ shift, int64_t film_ld,
                     const float* __restrict__ S1, const float* __restrict__ S2, const bf16_t* __restrict__ dx_add,
                     bf16_t* __restrict__ dx, int HW, int C, int G, int nchunk, GnsGeom gm) {
    const int item = gridDim.x - 1 - blockIdx.x;             // the sums pass went 0 .. n-1: start on what it read last
    const int t = threadIdx.x, b = item / nchunk, chunk = item - b * nchunk;
    if (t >= gm.nt) return;
    const int oct = t % gm.C8, rl = t / gm.C8, c0 = oct * 8, cg = C / G;
    const int r0 = chunk * gm.rows, r1 = r0 + gm.rows < HW ? r0 + gm.rows : HW;
    const int64_t sample = (int64_t)b * HW * C;
    const bf16_t *xs = x + sample, *ds = dout + sample, *as = dx_add + sample;
    bf16_t* os = dx + sample;
    const float invn = 1.f / ((float)cg * HW);
    float P[8], Q[8], mu[8], rs[8], K2[8], K3[8];
    gns_coef<FILM>(mean, rstd, gamma, beta, scale, shift, film_ld, b, c0, cg, G, P, Q, mu, rs);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int g = (c0 + j) / cg;
        K3[j] = rs[j] * rs[j] * (S2[b * G + g] * invn);
        K2[j] = rs[j] * (S1[b * G + g] * invn) - K3[j] * mu[j];
    }
    for (int rb = r0 + rl; rb < r1; rb += U * gm.rpi) {
        gns_u32x4 xv[U], dv[U], av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r = rb + u * gm.rpi;
            r = r < r1 ? r : r1 - 1;
            xv[u] = gns_ld_nt(xs + (unsigned)(r * C + c0));
            dv[u] = gns_ld_nt(ds + (unsigned)(r * C + c0));
            if (ADD) av[u] = gns_ld_nt(as + (unsigned)(r * C + c0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = rb + u * gm.rpi;
            float xf[8], df[8], af[8], o[8];
            gns_unpack(xv[u], xf);
            gns_unpack(dv[u], df);
            if (ADD) gns_unpack(av[u], af);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = df[j];
                if (SILU) d *= gn_silu_grad(xf[j] * P[j] + Q[j]);
                float v = P[j] * d - K3[j] * xf[j] - K2[j];
                if (ADD) v += af[j];
                o[j] = v;
            }
            if (r < r1) gns_st_nt(os + (unsigned)(r * C + c0), o);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Launch plan and C ABI
// ---------------------------------------------------------------------------------------------
static int g_gn_flat = -1;       // vaw_debug_gn_flat: -1 flat by shape, 0 never, 1 wherever the flat kernels can run (tests)
extern "C" void vaw_debug_gn_flat(int mode) { g_gn_flat = mode; }

extern "C" int64_t vaw_groupnorm_workspace_floats(int B, int HW, int C) {
    return (int64_t)4 * ceil_div(HW, GN_ROWS / 4) * B * C + (int64_t)4 * B * C + 2 * (int64_t)B * 64 + 64;   // the flat kernels' smallest chunks
}

// flat chunk rows: GN_ROWS, or less while that leaves fewer than two workgroups per CU; 0: the quad-mapped kernels
static int gn_flat_rows(vaw_dtype dt, int B, int HW, int C, int G) {
    const int mode = g_gn_flat;
    if (mode == 0 || dt != VAW_BF16 || C % 8 || C / 8 > GNS_NT || C > 2048 || C % G || (int64_t)B * HW >= (1 << 30) ||
        (int64_t)HW * C >= ((int64_t)1 << 31))
        return 0;
    for (int rows = GN_ROWS; rows >= GN_ROWS / 4; rows /= 2)
        if ((int64_t)B * ceil_div(HW, rows) >= 512) return rows;
    return mode == 1 ? GN_ROWS / 4 : 0;
}

extern "C" int vaw_gn_plan(int pass, vaw_dtype dt, int B, int HW, int C, int G, vaw_gn_launch* out) {
    VAW_CHECK_ARG(out, "gn_plan: null output");
    *out = vaw_gn_launch{};
    out->status = VAW_ERR_INVALID;
    out->off_part = out->off_sums = out->off_s1 = out->off_s2 = -1;
    VAW_CHECK_ARG(pass >= VAW_GN_FWD_SUMS && pass <= VAW_GN_BWD_APPLY, "gn_plan: unknown pass %d", pass);
    // refusals carry the name of the entry point the pass belongs to: they are what it returns
    const char* who = pass == VAW_GN_FWD_SUMS ? "groupnorm_fwd" : pass == VAW_GN_APPLY ? "groupnorm_apply" : "groupnorm_bwd";
    VAW_CHECK_ARG(dt == VAW_F32 || dt == VAW_BF16, "%s: dtype must be f32 or bf16", who);
    VAW_CHECK_ARG(B > 0 && HW > 0 && C > 0 && G > 0, "%s: sizes must be positive (B=%d HW=%d C=%d G=%d)", who, B, HW, C, G);
    VAW_CHECK_ARG(C % 4 == 0 && C % G == 0 && G <= 64, "%s: needs C %% 4 == 0, C %% G == 0, G <= 64 (C=%d G=%d)", who, C, G);
    VAW_CHECK_ARG(B < 65536, "%s: B=%d must be below 65536", who, B);
    const int flat_rows = gn_flat_rows(dt, B, HW, C, G);
    out->variant = flat_rows ? VAW_GNV_FLAT : VAW_GNV_QUAD;
    out->rows = flat_rows ? flat_rows : GN_ROWS;
    out->nch = ceil_div(HW, out->rows);
    out->block = 256;
    const bool sums = pass == VAW_GN_FWD_SUMS || pass == VAW_GN_BWD_SUMS;
    const int planes = pass == VAW_GN_FWD_SUMS ? 2 : 4;              // partial sums per (chunk, sample, channel)
    if (flat_rows) {
        out->nt = (GNS_NT / (C / 8)) * (C / 8);
        out->rpi = out->nt / (C / 8);
        out->grid_x = B * out->nch;
        out->grid_y = out->grid_z = 1;
        out->lds_bytes = sums ? (int64_t)sizeof(float) * (2 * GNS_NT * 8 + 2 * 2048) : 0;
    } else {
        VAW_CHECK_ARG(out->nch <= 65535, "%s: HW=%d is more than 65535 chunks of %d rows (grid.z)", who, HW, GN_ROWS);
        out->grid_x = ceil_div(C, 64);
        out->grid_y = B;
        out->grid_z = out->nch;
        out->lds_bytes = sums ? (int64_t)sizeof(float) * planes * 16 * 64 : 0;
    }
    // workspace: [planes][nch][B][C] chunk partials; backward: then the folded [4][B][C] sums and S1, S2 [B*G]
    const int64_t BC = (int64_t)B * C;
    if (sums) out->off_part = 0;
    if (pass == VAW_GN_FWD_SUMS) out->workspace_floats = planes * out->nch * BC;
    if (pass == VAW_GN_BWD_SUMS || pass == VAW_GN_BWD_APPLY) {
        if (sums) out->off_sums = planes * out->nch * BC;
        out->off_s1 = planes * out->nch * BC + 4 * BC;
        out->off_s2 = out->off_s1 + (int64_t)B * G;
        out->workspace_floats = out->off_s2 + (int64_t)B * G;
    }
    out->status = VAW_OK;
    return VAW_OK;
}

// runtime flags -> template arguments: f(std::bool_constant<flag>...)
template <bool... Bs, typename F>
static void gn_by_flags(F&& f) { f(std::bool_constant<Bs>{}...); }
template <bool... Bs, typename F, typename... Rest>
static void gn_by_flags(F&& f, bool flag, Rest... rest) {
    if (flag) gn_by_flags<Bs..., true>(f, rest...);
    else gn_by_flags<Bs..., false>(f, rest...);
}
static inline GnsGeom gns_geom(int C, const vaw_gn_launch& p) { return GnsGeom{C / 8, p.nt, p.rpi, p.rows}; }
static inline dim3 gn_grid(const vaw_gn_launch& p) { return dim3(p.grid_x, p.grid_y, p.grid_z); }

// Alignment the launch the plan chose assumes: the flat kernels move bf16 octets (16 bytes), the quad kernels channel quads (16 bytes
// of f32, 8 of bf16); gamma, beta and the FiLM rows are read as f32 quads by the quad kernels and are held to that on both mappings.
static inline bool gn_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static inline size_t gn_act_align(vaw_dtype dt, const vaw_gn_launch& p) { return p.variant == VAW_GNV_FLAT || dt == VAW_F32 ? 16 : 8; }
static int gn_check_params(const char* who, const float* gamma, const float* beta, const float* scale, const float* shift, int64_t film_ld) {
    VAW_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift go together", who);
    VAW_CHECK_ARG(!scale || film_ld % 4 == 0, "%s: film_ld must be a multiple of 4", who);
    VAW_CHECK_ARG(gn_aligned(gamma, 16) && gn_aligned(beta, 16), "%s: gamma and beta must be 16-byte aligned", who);
    VAW_CHECK_ARG(gn_aligned(scale, 16) && gn_aligned(shift, 16), "%s: scale and shift must be 16-byte aligned", who);
    return VAW_OK;
}

// The apply pass on given statistics: vaw_groupnorm_fwd's last launch and all of vaw_groupnorm_apply, so one plan by construction.
static int gn_apply_launch(const char* who, vaw_dtype dt, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           const float* scale, const float* shift, int64_t film_ld, int silu, void* y, int B, int HW, int C, int G,
                           hipStream_t s) {
    vaw_gn_launch p;
    if (int rc = vaw_gn_plan(VAW_GN_APPLY, dt, B, HW, C, G, &p)) return rc;
    VAW_CHECK_ARG(gn_aligned(x, gn_act_align(dt, p)) && gn_aligned(y, gn_act_align(dt, p)), "%s: x and y must be %d-byte aligned", who,
                  (int)gn_act_align(dt, p));
    if (p.variant == VAW_GNV_FLAT) {
        gn_by_flags([&](auto S, auto F) {
            gns_apply_kernel<4, S.value, F.value><<<gn_grid(p), p.block, 0, s>>>((const bf16_t*)x, mean, rstd, gamma, beta, scale, shift, film_ld,
                                                                                (bf16_t*)y, HW, C, G, p.nch, gns_geom(C, p));
        }, silu != 0, scale != nullptr);
    } else {
        BY_DTYPE(dt, (gn_apply_kernel<T><<<gn_grid(p), p.block, 0, s>>>((const T*)x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, (T*)y, HW, C, G)));
    }
    return VAW_OK;
}

extern "C" int vaw_groupnorm_fwd(vaw_dtype dt, const void* x, const float* gamma, const float* beta, const float* scale,
                                 const float* shift, int64_t film_ld, int silu, void* y, float* mean, float* rstd, int B,
                                 int HW, int C, int G, float eps, float* workspace, vaw_stream stream) {
    vaw_gn_launch p;
    if (int rc = vaw_gn_plan(VAW_GN_FWD_SUMS, dt, B, HW, C, G, &p)) return rc;
    VAW_CHECK_ARG(workspace, "groupnorm_fwd: null workspace");
    VAW_CHECK_ARG(x && y && gamma && beta && mean && rstd, "groupnorm_fwd: null pointer");
    if (int rc = gn_check_params("groupnorm_fwd", gamma, beta, scale, shift, film_ld)) return rc;
    VAW_CHECK_ARG(gn_aligned(x, gn_act_align(dt, p)) && gn_aligned(y, gn_act_align(dt, p)), "groupnorm_fwd: x and y must be %d-byte aligned",
                  (int)gn_act_align(dt, p));
    hipStream_t s = (hipStream_t)stream;
    float* part = workspace + p.off_part;
    if (p.variant == VAW_GNV_FLAT) {
        gns_fwd_sums_kernel<8><<<gn_grid(p), p.block, 0, s>>>((const bf16_t*)x, HW, C, B, p.nch, gns_geom(C, p), part);
    } else {
        BY_DTYPE(dt, (gn_fwd_sums_kernel<T><<<gn_grid(p), p.block, 0, s>>>((const T*)x, HW, C, B, p.nch, part)));
    }
    gn_group_stats_kernel<<<ceil_div(B * G, 128), 128, 0, s>>>(part, p.nch, B, C, G, HW, eps, mean, rstd);
    if (int rc = gn_apply_launch("groupnorm_fwd", dt, x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, y, B, HW, C, G, s)) return rc;
    VAW_CHECK_LAUNCH("groupnorm_fwd");
    return VAW_OK;
}

extern "C" int vaw_groupnorm_apply(vaw_dtype dt, const void* x, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, const float* scale, const float* shift, int64_t film_ld, int silu, void* y,
                                   int B, int HW, int C, int G, vaw_stream stream) {
    VAW_CHECK_ARG(x && y && mean && rstd && gamma && beta, "groupnorm_apply: null pointer");
    if (int rc = gn_check_params("groupnorm_apply", gamma, beta, scale, shift, film_ld)) return rc;
    if (int rc = gn_apply_launch("groupnorm_apply", dt, x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, y, B, HW, C, G, (hipStream_t)stream)) return rc;
    VAW_CHECK_LAUNCH("groupnorm_apply");
    return VAW_OK;
}

extern "C" int vaw_groupnorm_bwd(vaw_dtype dt, const void* dout, const void* x, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const float* scale, const float* shift,
                                 int64_t film_ld, int silu, const void* dx_add, void* dx, float* dgamma, float* dbeta,
                                 float grad_beta, float* dscale, float* dshift, int64_t dfilm_ld, int B, int HW, int C, int G,
                                 float* workspace, vaw_stream stream) {
    vaw_gn_launch ps, pa;
    if (int rc = vaw_gn_plan(VAW_GN_BWD_SUMS, dt, B, HW, C, G, &ps)) return rc;
    if (int rc = vaw_gn_plan(VAW_GN_BWD_APPLY, dt, B, HW, C, G, &pa)) return rc;
    VAW_CHECK_ARG(workspace, "groupnorm_bwd: null workspace");
    VAW_CHECK_ARG(dout && x && mean && rstd && gamma && beta && dx && dgamma && dbeta, "groupnorm_bwd: null pointer");
    if (int rc = gn_check_params("groupnorm_bwd", gamma, beta, scale, shift, film_ld)) return rc;
    VAW_CHECK_ARG(!scale || (dscale && dshift), "groupnorm_bwd: FiLM needs shift, dscale, dshift");
    const size_t al = gn_act_align(dt, ps);
    VAW_CHECK_ARG(gn_aligned(dout, al) && gn_aligned(x, al) && gn_aligned(dx, al) && gn_aligned(dx_add, al),
                  "groupnorm_bwd: dout, x, dx and dx_add must be %d-byte aligned", (int)al);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BC = (int64_t)B * C;
    float *part = workspace + ps.off_part, *sums = workspace + ps.off_sums, *S1 = workspace + ps.off_s1, *S2 = workspace + ps.off_s2;
    const bool flat = ps.variant == VAW_GNV_FLAT;
    const bf16_t *xb = (const bf16_t*)x, *db = (const bf16_t*)dout;
    if (flat) {
        gn_by_flags([&](auto S, auto F) {
            gns_bwd_sums_kernel<4, S.value, F.value><<<gn_grid(ps), ps.block, 0, s>>>(db, xb, mean, rstd, gamma, beta, scale, shift, film_ld, HW, C, G,
                                                                                     B, ps.nch, gns_geom(C, ps), part);
        }, silu != 0, scale != nullptr);
    } else {
        BY_DTYPE(dt, (gn_bwd_sums_kernel<T><<<gn_grid(ps), ps.block, 0, s>>>((const T*)dout, (const T*)x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, HW, C, G, B, ps.nch, part)));
    }
    const int nb1 = (int)ceil_div(B * G, 256), nb2 = (int)ceil_div(C, 16), nb3 = scale && dscale ? (int)ceil_div(BC, 256) : 0;
    gn_bwd_fold_kernel<<<ceil_div(4 * BC, 256), 256, 0, s>>>(part, ps.nch, B, C, sums);
    gn_bwd_group_kernel<<<nb1 + nb2 + nb3, 256, 0, s>>>(sums, gamma, B, C, G, S1, S2, dgamma, dbeta, grad_beta, scale ? dscale : nullptr, dshift,
                                                         dfilm_ld, nb1, nb2);
    if (flat) {
        gn_by_flags([&](auto S, auto F, auto A) {
            gns_bwd_apply_kernel<4, S.value, F.value, A.value><<<gn_grid(pa), pa.block, 0, s>>>(db, xb, mean, rstd, gamma, beta, scale, shift, film_ld,
                                                                                               S1, S2, (const bf16_t*)dx_add, (bf16_t*)dx, HW, C, G,
                                                                                               pa.nch, gns_geom(C, pa));
        }, silu != 0, scale != nullptr, dx_add != nullptr);
    } else {
        BY_DTYPE(dt, (gn_bwd_apply_kernel<T><<<gn_grid(pa), pa.block, 0, s>>>((const T*)dout, (const T*)x, mean, rstd, gamma, beta, scale, shift, film_ld, silu, S1, S2, (const T*)dx_add, (T*)dx, HW, C, G)));
    }
    VAW_CHECK_LAUNCH("groupnorm_bwd");
    return VAW_OK;
}

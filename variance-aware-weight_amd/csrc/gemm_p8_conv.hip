// Implicit-GEMM conv3x3 on the persistent kernel (gemm_p8_kernel.h, CONV modes): instantiations and the host entry that
// vaw_conv3x3 (gemm.hip) tries first.  Reference: the 3x3 convolutions of ResBlock / stem / head, models/unet.py:182-213,492,625.
#include "gemm_p8_kernel.h"
#include "gemm_plan.h"


// out[n][m] = beta * out[n][m] + sum_s slab[s][m][n]: the slab reduce of the transposed weight-gradient problem
// (slab rows = (tap, ci), columns = co; out = dW [Co][9*Ci]).  32 (m) x 64 (n) tiles: 16-byte slab reads (16 lanes per 256-byte row
// piece), the sums transposed through LDS, 16-byte writes of four consecutive m (8 lanes per 128-byte output row piece).  Nt % 4 == 0,
// Mt % 4 == 0 (9 Ci with Ci % 8 == 0).  (r3: the 4-byte version read 50 MB of slabs at 2.2 TB/s, 23 us per conv launch.)
__global__ void __launch_bounds__(256)
p8_conv_wgrad_reduce_kernel(const float* __restrict__ slab, int S, int Mt, int Nt, float* __restrict__ out, float beta,
                            const float* __restrict__ rowpart, float* __restrict__ bias_out, float bias_beta) {
    __shared__ float tile[32][65];
    if (rowpart && blockIdx.x == 0 && blockIdx.y == 0) {      // the bias gradient: fold the per-split column sums of dy, fixed order
        for (int n = threadIdx.x; n < Nt; n += blockDim.x) {
            float t = 0.f;
            for (int sp = 0; sp < S; ++sp) t += rowpart[(int64_t)sp * Nt + n];
            bias_out[n] = (bias_beta != 0.f ? bias_beta * bias_out[n] : 0.f) + t;
        }
    }
    const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 64;
    {
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;          // 16 lanes x 4 columns, 16 rows per pass
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = pass * 16 + ty, m = m0 + r, n = n0 + 4 * tx;
            f32x4 acc = {0, 0, 0, 0};
            if (m < Mt && n < Nt) {
                const float* p = slab + (int64_t)m * Nt + n;
                const int64_t plane = (int64_t)Mt * Nt;
                for (int sp = 0; sp < S; ++sp) acc += load4(p + sp * plane);
            }
            tile[r][4 * tx] = acc[0]; tile[r][4 * tx + 1] = acc[1]; tile[r][4 * tx + 2] = acc[2]; tile[r][4 * tx + 3] = acc[3];
        }
    }
    __syncthreads();
    {
        const int mq = threadIdx.x & 7, nr = threadIdx.x >> 3;           // 8 lanes x 4 consecutive m, 32 output rows (n) per pass
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int nl = pass * 32 + nr, n = n0 + nl, m = m0 + 4 * mq;
            if (n < Nt && m < Mt) {
                float* o = out + (int64_t)n * Mt + m;
                f32x4 v = {tile[4 * mq][nl], tile[4 * mq + 1][nl], tile[4 * mq + 2][nl], tile[4 * mq + 3][nl]};
                if (beta != 0.f) v += beta * load4(o);
                store4(o, v);
            }
        }
    }
}

// mode 0 forward, 1 input gradient, 2 weight gradient: the launch vaw_conv3x3_plan chose (variant VAW_GV_PERSISTENT), carried out.
void vaw_p8_conv(const vaw_conv3x3_launch& p, int mode, const bf16_t* act, const bf16_t* act2, const bf16_t* w, void* out, int H, int W,
                 int Ci, int Co, EpiDev e, float* workspace, hipStream_t s, float* bias_grad, float bias_beta) {
    const int64_t M = p.M, N = p.N;        // mode 2: the transposed problem, M = 9 Ci, N = Co
    const int bn = 64 * p.ntw, tiles_m = (int)((M + 255) / 256), tiles_n = (int)((N + bn - 1) / bn), nk = (int)(p.K / 64);
    const P8Conv cg{H, W, Ci, Co};
    e.M = M; e.N = N; e.ldc = N; e.C = out; e.slab = workspace; e.colpart = nullptr; e.rowpart = nullptr; e.nt_off = 1;
    if (p.bias_grad == VAW_CVB_FUSED) e.rowpart = workspace + (int64_t)p.split * M * N;      // behind the slabs
#define P8C(AKv, BKv, EPIv, CV, a, lda, b, ldb)                                                                                   \
    do {                                                                                                                          \
        if (p.ntw == 4) p8_launch_conv<AKv, BKv, 4, EPIv, CV>(a, lda, b, ldb, nk, tiles_m, tiles_n, p.split, p.grid_x, e, cg, s); \
        else p8_launch_conv<AKv, BKv, 3, EPIv, CV>(a, lda, b, ldb, nk, tiles_m, tiles_n, p.split, p.grid_x, e, cg, s);             \
    } while (0)
    if (mode == 0) {
        if (p.epi_kind == P8_RESID) P8C(true, true, P8_RESID, 1, act, (int64_t)Ci, w, 9LL * Ci);
        else P8C(true, true, P8_STORE, 1, act, (int64_t)Ci, w, 9LL * Ci);
    } else if (mode == 1) {
        P8C(true, false, P8_STORE, 2, act, (int64_t)Co, w, 9LL * Ci);
    } else {
        const float beta = e.beta;
        P8C(false, false, P8_SLAB, 3, act2, (int64_t)Ci, act, (int64_t)Co);      // A = x (gathered), B = dy
        dim3 grid((unsigned)((M + 31) / 32), (unsigned)((N + 63) / 64));
        p8_conv_wgrad_reduce_kernel<<<grid, 256, 0, s>>>(workspace, p.split, (int)M, (int)N, (float*)out, beta, e.rowpart, bias_grad, bias_beta);
    }
}

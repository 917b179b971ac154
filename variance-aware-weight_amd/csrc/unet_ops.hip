// UNet-side kernels (reference models/unet.py + tools/nn.py), all on NHWC ("pixels x channels") activations so
// that every conv is a GEMM over M = B*H*W pixel rows and the attention qkv rows are token-major (GroupNorm: groupnorm.hip):
//   im2col / col2im for conv3x3 pad 1 (round 1: explicit patch matrix, GEMM does the arithmetic)
//   2x2 average pool, nearest x2 upsample (+ their transposes), channel concat / split, NCHW <-> NHWC
// All HBM-bound, 4 channels per thread (16 B f32 / 8 B bf16), reductions in a fixed order (no float atomics).
#include <stdlib.h>

#include "common.h"

static inline int sgrid(int64_t work, int block) {
    int64_t g = (work + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
#define BY_DTYPE(dt, CALL)                      \
    if (dt == VAW_F32) { using T = float; CALL; } \
    else { using T = bf16_t; CALL; }
#define GRID_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---------------------------------------------------------------------------------------------
// conv3x3 (stride 1, pad 1) patch matrix: col[m, tap*C + c] = x[pixel(m) + (tap/3-1, tap%3-1), c]  (0 outside)
// col2im is its transpose as a GATHER: dx[p, c] = sum_tap dcol[p - shift(tap), tap*C + c]
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void im2col3x3_kernel(const T* __restrict__ x, T* __restrict__ col, int B, int H, int W, int C) {
    const int64_t total = (int64_t)B * H * W * 9 * (C / V);
    GRID_STRIDE(i, total) {
        const int cv = (int)(i % (C / V));
        int64_t r = i / (C / V);
        const int tap = (int)(r % 9);
        const int64_t m = r / 9;
        const int w = (int)(m % W), h = (int)((m / W) % H);
        const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
        T* dst = col + (m * 9 + tap) * C + cv * V;
        const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
        const T* src = x + (m + (int64_t)(tap / 3 - 1) * W + (tap % 3 - 1)) * C + cv * V;
        if (V == 4) {
            store4(dst, in ? load4(src) : f32x4{0, 0, 0, 0});
        } else {
            dst[0] = in ? src[0] : from_f32<T>(0.f);
        }
    }
}

template <typename T, int V>
__global__ void col2im3x3_kernel(const T* __restrict__ dcol, T* __restrict__ dx, int B, int H, int W, int C) {
    const int64_t total = (int64_t)B * H * W * (C / V);
    GRID_STRIDE(i, total) {
        const int cv = (int)(i % (C / V));
        const int64_t p = i / (C / V);
        const int w = (int)(p % W), h = (int)((p / W) % H);
        f32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dh = tap / 3 - 1, dw = tap % 3 - 1;
            const int hh = h - dh, ww = w - dw;     // the pixel whose patch holds p at position `tap`
            if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
                const T* src = dcol + ((p - (int64_t)dh * W - dw) * 9 + tap) * C + cv * V;
                if (V == 4) acc += load4(src);
                else acc[0] += to_f32(src[0]);
            }
        }
        if (V == 4) store4(dx + p * C + cv * 4, acc);
        else dx[p * C + cv] = from_f32<T>(acc[0]);
    }
}

// ---------------------------------------------------------------------------------------------
// conv3x3 weight gradient when one side has <= 4 channels (the 3-channel stem and output convs): a GEMM would
// have a 3- or 27-wide dimension.  One thread per channel of the WIDE side keeps its 9*S accumulators (S = small
// channel count) in registers and walks a chunk of pixels; chunk partials are folded in a fixed order.
//   SMALL_IN : dW[co][tap][ci] = sum_m dy[m][co] * x[nbr(m,tap)][ci],  thread = co, ci < S
//   !SMALL_IN: same sum, thread = ci, co < S
// ---------------------------------------------------------------------------------------------
#define WG_CHUNK 256
template <typename T, int S, bool SMALL_IN>
__global__ void __launch_bounds__(256)
conv3x3_wgrad_small_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part, int B, int H, int W,
                           int Cw /* wide channel count */) {
    // Per workgroup: WG_CHUNK pixels x 256 wide channels.  What every thread needs of a pixel -- the 3x3 x S patch of the
    // narrow input (SMALL_IN) or the S narrow output gradients plus the tap validity (SMALL_OUT) -- is gathered ONCE into
    // LDS by thread = pixel and then read back as broadcasts, instead of 256 threads re-loading the same scalars.
    constexpr int PS = SMALL_IN ? (9 * S + 3) / 4 * 4 : 4;
    __shared__ __attribute__((aligned(16))) float pix[WG_CHUNK][PS];
    __shared__ unsigned short tapmask[WG_CHUNK];             // bit t: tap t of this pixel lies inside the image
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int64_t M = (int64_t)B * H * W;
    const int64_t m0 = (int64_t)blockIdx.x * WG_CHUNK, m1 = m0 + WG_CHUNK < M ? m0 + WG_CHUNK : M;
    {
        const int64_t m = m0 + threadIdx.x;
        const int w = (int)(m % W), h = (int)((m / W) % H);
        unsigned mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
            const bool ok = m < M && hh >= 0 && hh < H && ww >= 0 && ww < W;
            mask |= ok ? (1u << t) : 0u;
            if (SMALL_IN) {
                const T* xp = x + (m + (int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * S;
#pragma unroll
                for (int j = 0; j < S; ++j) pix[threadIdx.x][t * S + j] = ok ? to_f32(xp[j]) : 0.f;
            }
        }
        if (SMALL_IN) {
#pragma unroll
            for (int k = 9 * S; k < PS; ++k) pix[threadIdx.x][k] = 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pix[threadIdx.x][j] = (j < S && m < M) ? to_f32(dy[m * S + j]) : 0.f;
        }
        tapmask[threadIdx.x] = (unsigned short)mask;
    }
    __syncthreads();
    float acc[9][S];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < S; ++j) acc[t][j] = 0.f;
    if (c < Cw) {
        for (int64_t m = m0; m < m1; ++m) {
            const int lm = (int)(m - m0);
            if (SMALL_IN) {
                const float g = to_f32(dy[m * Cw + c]);
#pragma unroll
                for (int k4 = 0; k4 < PS / 4; ++k4) {
                    const f32x4 pv = load4(&pix[lm][4 * k4]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = 4 * k4 + u;
                        if (k < 9 * S) acc[k / S][k % S] += g * pv[u];       // padded taps hold zeros
                    }
                }
            } else {
                const f32x4 g = load4(&pix[lm][0]);
                const unsigned mask = tapmask[lm];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (mask & (1u << t)) {                  // uniform across the workgroup: same pixel for every thread
                        const float xv = to_f32(x[(m + (int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * Cw + c]);
#pragma unroll
                        for (int j = 0; j < S; ++j) acc[t][j] += g[j] * xv;
                    }
                }
            }
        }
        // partial layout = the weight layout [Co][9][Ci], one slab per chunk
        float* out = part + (int64_t)blockIdx.x * 9 * S * Cw;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (SMALL_IN) out[((int64_t)c * 9 + t) * S + j] = acc[t][j];
                else out[((int64_t)j * 9 + t) * Cw + c] = acc[t][j];
            }
    }
}
__global__ void fold_slabs_kernel(const float* __restrict__ part, int64_t nslab, int64_t n, float* __restrict__ out, float beta) {
    __shared__ float fold[8][33];
    const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;   // 32 outputs x 8 slab groups
    const int64_t i = (int64_t)blockIdx.x * 32 + cl;
    float acc = 0.f;
    if (i < n)
        for (int64_t sidx = grp; sidx < nslab; sidx += 8) acc += part[sidx * n + i];
    fold[grp][cl] = acc;
    __syncthreads();
    if (grp == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += fold[g][cl];
        out[i] = (beta != 0.f ? beta * out[i] : 0.f) + t;
    }
}

extern "C" int64_t vaw_conv3x3_wgrad_small_workspace_floats(int B, int H, int W, int Ci, int Co) {
    const int64_t M = (int64_t)B * H * W;
    return ((M + WG_CHUNK - 1) / WG_CHUNK) * 9 * Ci * Co;
}

extern "C" int vaw_conv3x3_wgrad_small(vaw_dtype dt, const void* dy, const void* x, float* dw, float beta, int B, int H, int W,
                                       int Ci, int Co, float* workspace, int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0 && (Ci <= 4 || Co <= 4), "conv3x3_wgrad_small: needs Ci<=4 or Co<=4");
    VAW_CHECK_ARG(workspace && workspace_floats >= vaw_conv3x3_wgrad_small_workspace_floats(B, H, W, Ci, Co), "conv3x3_wgrad_small: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = (int64_t)B * H * W;
    const int nchunk = (int)((M + WG_CHUNK - 1) / WG_CHUNK);
    const bool small_in = Ci <= 4;
    const int S = small_in ? Ci : Co, Cw = small_in ? Co : Ci;
    dim3 grid(nchunk, ceil_div(Cw, 256));
#define WG_LAUNCH(Sv)                                                                                                          \
    if (small_in) { BY_DTYPE(dt, (conv3x3_wgrad_small_kernel<T, Sv, true><<<grid, 256, 0, s>>>((const T*)dy, (const T*)x, workspace, B, H, W, Cw))); } \
    else { BY_DTYPE(dt, (conv3x3_wgrad_small_kernel<T, Sv, false><<<grid, 256, 0, s>>>((const T*)dy, (const T*)x, workspace, B, H, W, Cw))); }
    switch (S) {
        case 1: WG_LAUNCH(1) break;
        case 2: WG_LAUNCH(2) break;
        case 3: WG_LAUNCH(3) break;
        default: WG_LAUNCH(4) break;
    }
    const int64_t n = 9LL * Ci * Co;
    fold_slabs_kernel<<<ceil_div(n, 32), 256, 0, s>>>(workspace, nchunk, n, dw, beta);
    VAW_CHECK_LAUNCH("conv3x3_wgrad_small");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// conv3x3 with a narrow side (<= 4 channels): the 3-channel stem and the 3-channel output conv.  27 (or 36) taps
// per output are too short a K for the MFMA tile and the patch matrix would be pure HBM traffic, so these are direct
// f32-accumulating kernels: weights live in LDS as f32, activations are read once, outputs written in 16-byte pieces.
//   WIDE_OUT  in [M][S] -> out [M][Cw]; flip=0: forward (w = [Cw][9][S]);  flip=1: input gradient of a conv whose
//             OUTPUT is narrow: in = dy [M][S], out = dx [M][Cw], w = [S][9][Cw] read with the tap reversed
//   NARROW_OUT in [M][Cw] -> out [M][S], forward, w = [S][9][Cw]
// ---------------------------------------------------------------------------------------------
#define NW_PIX 2          // pixels per thread (the LDS weight reads are shared between them)
#define NW_BLOCK_PIX 256  // pixels per workgroup
template <typename T, int S>
__global__ void __launch_bounds__(256)
conv3x3_narrow_in_kernel(const T* __restrict__ in, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out,
                         int B, int H, int W, int Cw, int flip) {
    constexpr int PS = (9 * S + 3) / 4 * 4;          // patch row padded to whole 16-byte quads
    __shared__ float wl[9 * S][256 + 8];             // [tap*S + j][wide channel of this 256-chunk]
    __shared__ __attribute__((aligned(16))) float pat[NW_BLOCK_PIX][PS];   // the 3x3 x S patch of every pixel of the workgroup
    const int c0 = blockIdx.y * 256, cn = Cw - c0 < 256 ? Cw - c0 : 256;
    for (int i = threadIdx.x; i < 9 * S * cn; i += 256) {
        const int c = i % cn, kj = i / cn, tap = kj / S, j = kj % S;
        wl[kj][c] = flip ? to_f32(w[((int64_t)j * 9 + (8 - tap)) * Cw + c0 + c]) : to_f32(w[((int64_t)(c0 + c) * 9 + tap) * S + j]);
    }
    const int64_t M = (int64_t)B * H * W;
    {   // thread t gathers the patch of pixel t once (zero padding resolved here); everyone then reads it from LDS
        const int64_t p = (int64_t)blockIdx.x * NW_BLOCK_PIX + threadIdx.x;
        const int wq = (int)(p % W), hq = (int)((p / W) % H);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int hh = hq + t / 3 - 1, ww = wq + t % 3 - 1;
            const bool ok = p < M && hh >= 0 && hh < H && ww >= 0 && ww < W;
            const T* src = in + (p + (int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * S;
#pragma unroll
            for (int j = 0; j < S; ++j) pat[threadIdx.x][t * S + j] = ok ? to_f32(src[j]) : 0.f;
        }
#pragma unroll
        for (int k = 9 * S; k < PS; ++k) pat[threadIdx.x][k] = 0.f;
    }
    __syncthreads();
    const int cg = (threadIdx.x & 31) * 8, pl = threadIdx.x >> 5;     // 32 groups of 8 channels x 8 pixel lanes
    if (cg >= cn) return;                                               // Cw % 8 == 0: a group is in or out as a whole
    f32x4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
    if (bias) { b0 = load4(bias + c0 + cg); b1 = load4(bias + c0 + cg + 4); }
    for (int it = 0; it < NW_BLOCK_PIX / (8 * NW_PIX); ++it) {
        const int lp = (it * 8 + pl) * NW_PIX;                          // first of this thread's pixels inside the workgroup
        const int64_t p0 = (int64_t)blockIdx.x * NW_BLOCK_PIX + lp;
        f32x4 a0[NW_PIX], a1[NW_PIX];
#pragma unroll
        for (int q = 0; q < NW_PIX; ++q) { a0[q] = b0; a1[q] = b1; }
#pragma unroll
        for (int k4 = 0; k4 < PS / 4; ++k4) {
            f32x4 pv[NW_PIX];
#pragma unroll
            for (int q = 0; q < NW_PIX; ++q) pv[q] = load4(&pat[lp + q][4 * k4]);       // same address for the 32 channel groups: broadcast
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kj = 4 * k4 + u;
                if (kj >= 9 * S) break;
                const f32x4 w0 = load4(&wl[kj][cg]), w1 = load4(&wl[kj][cg + 4]);
#pragma unroll
                for (int q = 0; q < NW_PIX; ++q) {
                    a0[q] += pv[q][u] * w0;
                    a1[q] += pv[q][u] * w1;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NW_PIX; ++q)
            if (p0 + q < M) {
                T* dst = out + (p0 + q) * Cw + c0 + cg;
                store4(dst, a0[q]);
                store4(dst + 4, a1[q]);
            }
    }
}

template <typename T, int S>
__global__ void __launch_bounds__(256)
conv3x3_narrow_out_kernel(const T* __restrict__ in, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out,
                          int B, int H, int W, int Cw) {
    extern __shared__ float wsm[];                   // [S][9][Cw] f32
    for (int i = threadIdx.x; i < S * 9 * Cw; i += 256) wsm[i] = to_f32(w[i]);
    __syncthreads();
    const int sub = threadIdx.x & 7;                 // 8 lanes share a pixel, each takes every 8th 8-channel chunk
    const int64_t M = (int64_t)B * H * W;
    const int64_t p = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = p < M;
    const int wq = live ? (int)(p % W) : 0, hq = live ? (int)((p / W) % H) : 0;
    float acc[S];
#pragma unroll
    for (int j = 0; j < S; ++j) acc[j] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int hh = hq + t / 3 - 1, ww = wq + t % 3 - 1;
        if (!(live && hh >= 0 && hh < H && ww >= 0 && ww < W)) continue;
        const T* src = in + (p + (int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * Cw;
        for (int c = sub * 8; c < Cw; c += 64) {
            const f32x4 x0 = load4(src + c), x1 = load4(src + c + 4);
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const float* wr = wsm + ((int64_t)j * 9 + t) * Cw + c;
                const f32x4 w0 = load4(wr), w1 = load4(wr + 4);
                acc[j] += ((x0[0] * w0[0] + x0[1] * w0[1]) + (x0[2] * w0[2] + x0[3] * w0[3])) +
                          ((x1[0] * w1[0] + x1[1] * w1[1]) + (x1[2] * w1[2] + x1[3] * w1[3]));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
        acc[j] += __shfl_xor(acc[j], 1, 64);
        acc[j] += __shfl_xor(acc[j], 2, 64);
        acc[j] += __shfl_xor(acc[j], 4, 64);
    }
    if (live && sub == 0) {
#pragma unroll
        for (int j = 0; j < S; ++j) out[p * S + j] = from_f32<T>(acc[j] + (bias ? bias[j] : 0.f));
    }
}

template <typename T, int S>
static void launch_narrow_out(const T* in, const T* w, const float* bias, T* out, int B, int H, int W, int Cw, int64_t M,
                              size_t lds, hipStream_t s) {
    (void)hipFuncSetAttribute((const void*)conv3x3_narrow_out_kernel<T, S>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    conv3x3_narrow_out_kernel<T, S><<<ceil_div(M, 32), 256, lds, s>>>(in, w, bias, out, B, H, W, Cw);
}

extern "C" int vaw_conv3x3_narrow(vaw_dtype dt, int mode, const void* in, const void* w, const float* bias, void* out, int B, int H,
                                  int W, int Cn, int Cw, vaw_stream stream) {
    VAW_CHECK_ARG(mode >= 0 && mode <= 2 && in && w && out && B > 0 && H > 0 && W > 0 && Cn > 0 && Cw > 0, "conv3x3_narrow: bad arguments");
    if (Cn > 4 || Cw % 8 || (mode == 2 && (int64_t)Cn * 9 * Cw * 4 > 96 * 1024)) return VAW_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = (int64_t)B * H * W;
    if (mode == 2) {
        const size_t lds = (size_t)Cn * 9 * Cw * 4;
#define NO_LAUNCH(Sv) BY_DTYPE(dt, (launch_narrow_out<T, Sv>((const T*)in, (const T*)w, bias, (T*)out, B, H, W, Cw, M, lds, s)))
        switch (Cn) {
            case 1: NO_LAUNCH(1); break;
            case 2: NO_LAUNCH(2); break;
            case 3: NO_LAUNCH(3); break;
            default: NO_LAUNCH(4); break;
        }
    } else {
        dim3 grid(ceil_div(M, NW_BLOCK_PIX), ceil_div(Cw, 256));
#define NI_LAUNCH(Sv) \
    BY_DTYPE(dt, (conv3x3_narrow_in_kernel<T, Sv><<<grid, 256, 0, s>>>((const T*)in, (const T*)w, bias, (T*)out, B, H, W, Cw, mode)))
        switch (Cn) {
            case 1: NI_LAUNCH(1); break;
            case 2: NI_LAUNCH(2); break;
            case 3: NI_LAUNCH(3); break;
            default: NI_LAUNCH(4); break;
        }
    }
    VAW_CHECK_LAUNCH("conv3x3_narrow");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// resampling, concat, layout
// ---------------------------------------------------------------------------------------------
// mode 0: out[b,h,w,:] = mean of the 2x2 block of in (in is 2H x 2W)          (avg_pool2d; also nearest-upsample^T * 1/4 * 4)
// mode 1: out[b,h,w,:] = in[b,h/2,w/2,:] * s                                     (nearest x2; also avg_pool^T with s = 1/4)
template <typename T>
__global__ void resample2_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int Ho, int Wo, int C, int mode, float s) {
    const int64_t total4 = (int64_t)B * Ho * Wo * C / 4;
    GRID_STRIDE(i, total4) {
        const int64_t e = 4 * i;
        const int c = (int)(e % C);
        int64_t r = e / C;
        const int w = (int)(r % Wo), h = (int)((r / Wo) % Ho), b = (int)(r / ((int64_t)Wo * Ho));
        f32x4 v;
        if (mode == 0) {
            const int Wi = 2 * Wo;
            const T* p = in + (((int64_t)b * 2 * Ho + 2 * h) * Wi + 2 * w) * C + c;
            v = ((load4(p) + load4(p + C)) + load4(p + (int64_t)Wi * C)) + load4(p + (int64_t)Wi * C + C);
            v *= s;
        } else {
            const int Wi = Wo / 2;
            v = load4(in + (((int64_t)b * (Ho / 2) + h / 2) * Wi + w / 2) * C + c) * s;
        }
        store4(out + e, v);
    }
}

// out[m, 0:Ca] = a[m,:], out[m, Ca:Ca+Cb] = b[m,:]   (split = the inverse; ADD accumulates into a/b instead of overwriting)
template <typename T, bool SPLIT>
__global__ void concat_kernel(T* __restrict__ a, T* __restrict__ b, T* __restrict__ cat, int64_t M, int Ca, int Cb) {
    const int C = Ca + Cb;
    const int64_t total4 = M * C / 4;
    GRID_STRIDE(i, total4) {
        const int64_t e = 4 * i;
        const int c = (int)(e % C);
        const int64_t m = e / C;
        T* side = c < Ca ? a + m * Ca + c : b + m * Cb + (c - Ca);
        if (SPLIT) store4(side, load4(cat + e));
        else store4(cat + e, load4(side));
    }
}

template <typename T>
__global__ void add_kernel(T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
    GRID_STRIDE(i, n / 4) store4(dst + 4 * i, load4(dst + 4 * i) + load4(src + 4 * i));
}

// bf16 fast paths of the three data-movement kernels above (2x2 pool / nearest x2, channel concat / split, gradient add) on
// 16-byte accesses with U independent octets in flight per lane and non-temporal stores: they are pure HBM passes and ran at
// ~4 TB/s on 8-byte accesses with one load in flight and a 64-bit division per element.  Same arithmetic, same order.
#define MV_U 4
__device__ __forceinline__ void mv_unpack(gns_u32x4 v, float (&f)[8]) { gns_unpack(v, f); }
__device__ __forceinline__ gns_u32x4 mv_pack(const float (&f)[8]) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16_t)f[j];
    return __builtin_bit_cast(gns_u32x4, v);
}
__global__ void __launch_bounds__(256)
add8_kernel(bf16_t* __restrict__ dst, const bf16_t* __restrict__ src, unsigned n8) {
    for (unsigned base = blockIdx.x * (256u * MV_U); base < n8; base += gridDim.x * (256u * MV_U)) {
        gns_u32x4 a[MV_U], b[MV_U];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x, ic = i < n8 ? i : n8 - 1;
            a[u] = *reinterpret_cast<const gns_u32x4*>(dst + 8ull * ic);
            b[u] = gns_ld_nt(src + 8ull * ic);
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x;
            float x[8], y[8];
            mv_unpack(a[u], x);
            mv_unpack(b[u], y);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] += y[j];
            if (i < n8) *reinterpret_cast<gns_u32x4*>(dst + 8ull * i) = mv_pack(x);
        }
    }
}
template <bool SPLIT>
__global__ void __launch_bounds__(256)
concat8_kernel(bf16_t* __restrict__ a, bf16_t* __restrict__ b, bf16_t* __restrict__ cat, unsigned n8, unsigned Ca8, unsigned Cb8) {
    const unsigned C8 = Ca8 + Cb8;
    for (unsigned base = blockIdx.x * (256u * MV_U); base < n8; base += gridDim.x * (256u * MV_U)) {
        gns_u32x4 v[MV_U];
        bf16_t* side[MV_U];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x, ic = i < n8 ? i : n8 - 1;
            const unsigned m = ic / C8, c = ic - m * C8;
            side[u] = c < Ca8 ? a + 8ull * ((uint64_t)m * Ca8 + c) : b + 8ull * ((uint64_t)m * Cb8 + (c - Ca8));
            v[u] = SPLIT ? gns_ld_nt(cat + 8ull * ic) : gns_ld_nt(side[u]);
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x;
            if (i < n8) {
                if (SPLIT) *reinterpret_cast<gns_u32x4*>(side[u]) = v[u];
                else *reinterpret_cast<gns_u32x4*>(cat + 8ull * i) = v[u];
            }
        }
    }
}
template <int MODE>       // 0: 2x2 mean pool (out = Ho x Wo from 2Ho x 2Wo), 1: nearest x2 (out = Ho x Wo from Ho/2 x Wo/2); both times s
__global__ void __launch_bounds__(256)
resample8_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, unsigned n8, unsigned Ho, unsigned Wo, unsigned C8, float s) {
    for (unsigned base = blockIdx.x * (256u * MV_U); base < n8; base += gridDim.x * (256u * MV_U)) {
        gns_u32x4 v[MV_U][MODE == 0 ? 4 : 1];
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x, ic = i < n8 ? i : n8 - 1;
            const unsigned r = ic / C8, c = ic - r * C8, w = r % Wo, hb = r / Wo, h = hb % Ho, b = hb / Ho;
            if (MODE == 0) {
                const unsigned Wi = 2 * Wo;
                const bf16_t* p = in + 8ull * ((((uint64_t)b * 2 * Ho + 2 * h) * Wi + 2 * w) * C8 + c);
                v[u][0] = gns_ld_nt(p);
                v[u][1] = gns_ld_nt(p + 8ull * C8);
                v[u][2] = gns_ld_nt(p + 8ull * Wi * C8);
                v[u][3] = gns_ld_nt(p + 8ull * Wi * C8 + 8ull * C8);
            } else {
                const unsigned Wi = Wo / 2;
                v[u][0] = gns_ld(in + 8ull * ((((uint64_t)b * (Ho / 2) + h / 2) * Wi + w / 2) * C8 + c));
            }
        }
#pragma unroll
        for (int u = 0; u < MV_U; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x;
            float x[8];
            mv_unpack(v[u][0], x);
            if (MODE == 0) {
                float y[8], z[8], t[8];
                mv_unpack(v[u][1], y);
                mv_unpack(v[u][2], z);
                mv_unpack(v[u][MODE == 0 ? 3 : 0], t);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = ((x[j] + y[j]) + z[j]) + t[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] *= s;
            if (i < n8) __builtin_nontemporal_store(mv_pack(x), reinterpret_cast<gns_u32x4*>(out + 8ull * i));
        }
    }
}
static inline int mv_grid(int64_t n8) {
    const int64_t g = (n8 + 256 * MV_U - 1) / (256 * MV_U);
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
static bool mv_fast(vaw_dtype dt, int64_t n8) {
    static int on = -1;
    if (on < 0) {
        const char* v = getenv("VAW_MOVE8");
        on = v ? (atoi(v) != 0) : 1;
    }
    return on && dt == VAW_BF16 && n8 > 0 && n8 < ((int64_t)1 << 31);
}

// NCHW f32 <-> NHWC act dtype
template <typename T, bool TO_NHWC>
__global__ void layout_kernel(const float* __restrict__ nchw_in, float* __restrict__ nchw_out, const T* __restrict__ nhwc_in,
                              T* __restrict__ nhwc_out, int B, int C, int HW) {
    const int64_t total = (int64_t)B * C * HW;
    GRID_STRIDE(i, total) {
        const int p = (int)(i % HW);
        const int c = (int)((i / HW) % C);
        const int b = (int)(i / ((int64_t)HW * C));
        const int64_t j = ((int64_t)b * HW + p) * C + c;
        if (TO_NHWC) nhwc_out[j] = from_f32<T>(nchw_in[i]);
        else nchw_out[i] = to_f32(nhwc_in[j]);
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------

extern "C" int vaw_im2col3x3(vaw_dtype dt, const void* x, void* col, int B, int H, int W, int C, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "im2col3x3: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    if (C % 4 == 0) {
        const int64_t n = (int64_t)B * H * W * 9 * (C / 4);
        BY_DTYPE(dt, (im2col3x3_kernel<T, 4><<<sgrid(n, 256), 256, 0, s>>>((const T*)x, (T*)col, B, H, W, C)));
    } else {
        const int64_t n = (int64_t)B * H * W * 9 * C;
        BY_DTYPE(dt, (im2col3x3_kernel<T, 1><<<sgrid(n, 256), 256, 0, s>>>((const T*)x, (T*)col, B, H, W, C)));
    }
    VAW_CHECK_LAUNCH("im2col3x3");
    return VAW_OK;
}

extern "C" int vaw_col2im3x3(vaw_dtype dt, const void* dcol, void* dx, int B, int H, int W, int C, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "col2im3x3: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    if (C % 4 == 0) {
        const int64_t n = (int64_t)B * H * W * (C / 4);
        BY_DTYPE(dt, (col2im3x3_kernel<T, 4><<<sgrid(n, 256), 256, 0, s>>>((const T*)dcol, (T*)dx, B, H, W, C)));
    } else {
        const int64_t n = (int64_t)B * H * W * C;
        BY_DTYPE(dt, (col2im3x3_kernel<T, 1><<<sgrid(n, 256), 256, 0, s>>>((const T*)dcol, (T*)dx, B, H, W, C)));
    }
    VAW_CHECK_LAUNCH("col2im3x3");
    return VAW_OK;
}

extern "C" int vaw_resample2(vaw_dtype dt, const void* in, void* out, int B, int Ho, int Wo, int C, int mode, float s_,
                             vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && Ho > 0 && Wo > 0 && C % 4 == 0 && (mode == 0 || (mode == 1 && Ho % 2 == 0 && Wo % 2 == 0)), "resample2: bad sizes");
    const int64_t n4 = (int64_t)B * Ho * Wo * C / 4;
    if (C % 8 == 0 && mv_fast(dt, n4 / 2) && ((uintptr_t)in | (uintptr_t)out) % 16 == 0) {
        const unsigned n8 = (unsigned)(n4 / 2);
        if (mode == 0) resample8_kernel<0><<<mv_grid(n8), 256, 0, (hipStream_t)stream>>>((const bf16_t*)in, (bf16_t*)out, n8, Ho, Wo, C / 8, s_);
        else resample8_kernel<1><<<mv_grid(n8), 256, 0, (hipStream_t)stream>>>((const bf16_t*)in, (bf16_t*)out, n8, Ho, Wo, C / 8, s_);
        VAW_CHECK_LAUNCH("resample2");
        return VAW_OK;
    }
    BY_DTYPE(dt, (resample2_kernel<T><<<sgrid(n4, 256), 256, 0, (hipStream_t)stream>>>((const T*)in, (T*)out, B, Ho, Wo, C, mode, s_)));
    VAW_CHECK_LAUNCH("resample2");
    return VAW_OK;
}

extern "C" int vaw_concat_channels(vaw_dtype dt, void* a, void* b, void* cat, int64_t M, int Ca, int Cb, int split,
                                   vaw_stream stream) {
    VAW_CHECK_ARG(M > 0 && Ca > 0 && Cb > 0 && Ca % 4 == 0 && Cb % 4 == 0, "concat_channels: channel counts must be multiples of 4");
    const int64_t n4 = M * (Ca + Cb) / 4;
    hipStream_t s = (hipStream_t)stream;
    if (Ca % 8 == 0 && Cb % 8 == 0 && mv_fast(dt, n4 / 2) && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)cat) % 16 == 0) {
        const unsigned n8 = (unsigned)(n4 / 2);
        if (split) concat8_kernel<true><<<mv_grid(n8), 256, 0, s>>>((bf16_t*)a, (bf16_t*)b, (bf16_t*)cat, n8, Ca / 8, Cb / 8);
        else concat8_kernel<false><<<mv_grid(n8), 256, 0, s>>>((bf16_t*)a, (bf16_t*)b, (bf16_t*)cat, n8, Ca / 8, Cb / 8);
        VAW_CHECK_LAUNCH("concat_channels");
        return VAW_OK;
    }
    if (split) { BY_DTYPE(dt, (concat_kernel<T, true><<<sgrid(n4, 256), 256, 0, s>>>((T*)a, (T*)b, (T*)cat, M, Ca, Cb))); }
    else { BY_DTYPE(dt, (concat_kernel<T, false><<<sgrid(n4, 256), 256, 0, s>>>((T*)a, (T*)b, (T*)cat, M, Ca, Cb))); }
    VAW_CHECK_LAUNCH("concat_channels");
    return VAW_OK;
}

extern "C" int vaw_add_inplace(vaw_dtype dt, void* dst, const void* src, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(n > 0 && n % 4 == 0, "add_inplace: n must be a positive multiple of 4");
    if (n % 8 == 0 && mv_fast(dt, n / 8) && ((uintptr_t)dst | (uintptr_t)src) % 16 == 0) {
        add8_kernel<<<mv_grid(n / 8), 256, 0, (hipStream_t)stream>>>((bf16_t*)dst, (const bf16_t*)src, (unsigned)(n / 8));
        VAW_CHECK_LAUNCH("add_inplace");
        return VAW_OK;
    }
    BY_DTYPE(dt, (add_kernel<T><<<sgrid(n / 4, 256), 256, 0, (hipStream_t)stream>>>((T*)dst, (const T*)src, n)));
    VAW_CHECK_LAUNCH("add_inplace");
    return VAW_OK;
}

// ---- ResBlock variants off the factory path (reference models/unet.py:81-140, 206-256) -------------------------------
// out = a * b elementwise (act dtype): nn.Dropout with a pre-scaled keep mask, forward and backward alike
template <typename T>
__global__ void mul_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        store4(out + 4 * i, load4(a + 4 * i) * load4(b + 4 * i));
}
extern "C" int vaw_mul(vaw_dtype dt, const void* a, const void* b, void* out, int64_t n, vaw_stream stream) {
    VAW_CHECK_ARG(a && b && out && n > 0 && n % 4 == 0, "mul: n must be a positive multiple of 4");
    BY_DTYPE(dt, (mul_kernel<T><<<sgrid(n / 4, 256), 256, 0, (hipStream_t)stream>>>((const T*)a, (const T*)b, (T*)out, n / 4)));
    VAW_CHECK_LAUNCH("mul");
    return VAW_OK;
}

// nn.Dropout's keep mask at 1 bit per element (what a checkpointed ResBlock keeps).  Pack: a lane owns one 32-bit word = 32 mask
// elements, read with 16-byte loads (4 for bf16, 8 for f32), and writes it with one plain dword store.  Apply: a lane owns one mask
// BYTE = 8 elements (one 16-byte access of bf16, two of f32); the product is the f32 multiply and rounding of mul_kernel, with
// b = keep_scale or 0, so the result is bitwise vaw_mul's with the unpacked mask.
template <typename T> struct Vec16;
template <> struct Vec16<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <typename T>
__global__ void __launch_bounds__(256)
dropout_pack_kernel(const T* __restrict__ mask, unsigned* __restrict__ bits, int64_t n, int64_t nwords) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int V = Vec16<T>::N;
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = 32 * w;
        unsigned word = 0;
#pragma unroll
        for (int g = 0; g < 32 / V; ++g) {
            if (e0 + g * V < n) {                      // n % 8 == 0: a 16-byte group lies wholly inside or wholly outside
                const vec_t v = *reinterpret_cast<const vec_t*>(mask + e0 + g * V);
#pragma unroll
                for (int j = 0; j < V; ++j) word |= ((float)v[j] != 0.f ? 1u : 0u) << (g * V + j);
            }
        }
        bits[w] = word;
    }
}
template <typename T>
__global__ void __launch_bounds__(256)
dropout_bits_kernel(const T* __restrict__ x, const unsigned char* __restrict__ bits, float keep_scale, T* __restrict__ y, int64_t n8) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int V = Vec16<T>::N;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned m = bits[i];
#pragma unroll
        for (int g = 0; g < 8 / V; ++g) {
            const vec_t v = *reinterpret_cast<const vec_t*>(x + 8 * i + g * V);
            vec_t o;
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = from_f32<T>(to_f32(v[j]) * (((m >> (g * V + j)) & 1u) ? keep_scale : 0.f));
            *reinterpret_cast<vec_t*>(y + 8 * i + g * V) = o;
        }
    }
}
extern "C" int64_t vaw_dropout_bits_words(int64_t n) { return n > 0 ? (n + 31) / 32 : 0; }
extern "C" int vaw_dropout_pack(vaw_dtype dt, const void* mask, void* bits, int64_t M, int C, vaw_stream stream) {
    VAW_CHECK_ARG(mask && bits, "dropout_pack: null pointer");
    VAW_CHECK_ARG(dt == VAW_F32 || dt == VAW_BF16, "dropout_pack: dtype must be f32 or bf16");
    VAW_CHECK_ARG(M > 0 && C > 0 && C % 8 == 0, "dropout_pack: C must be a positive multiple of 8 (C=%d)", C);
    VAW_CHECK_ARG((uintptr_t)mask % 16 == 0 && (uintptr_t)bits % 4 == 0, "dropout_pack: mask must be 16-byte aligned, bits 4-byte");
    const int64_t n = M * C, nwords = vaw_dropout_bits_words(n);
    BY_DTYPE(dt, (dropout_pack_kernel<T><<<sgrid(nwords, 256), 256, 0, (hipStream_t)stream>>>((const T*)mask, (unsigned*)bits, n, nwords)));
    VAW_CHECK_LAUNCH("dropout_pack");
    return VAW_OK;
}
static int dropout_bits_apply(const char* what, vaw_dtype dt, const void* x, const void* bits, float keep_scale, void* y, int64_t n,
                              vaw_stream stream) {
    VAW_CHECK_ARG(x && bits && y, "%s: null pointer", what);
    VAW_CHECK_ARG(dt == VAW_F32 || dt == VAW_BF16, "%s: dtype must be f32 or bf16", what);
    VAW_CHECK_ARG(n > 0 && n % 8 == 0, "%s: n must be a positive multiple of 8", what);
    VAW_CHECK_ARG(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "%s: x and y must be 16-byte aligned", what);
    BY_DTYPE(dt, (dropout_bits_kernel<T><<<sgrid(n / 8, 256), 256, 0, (hipStream_t)stream>>>((const T*)x, (const unsigned char*)bits,
                                                                                             keep_scale, (T*)y, n / 8)));
    VAW_CHECK_LAUNCH(what);
    return VAW_OK;
}
extern "C" int vaw_dropout_bits_fwd(vaw_dtype dt, const void* x, const void* bits, float keep_scale, void* y, int64_t n, vaw_stream stream) {
    return dropout_bits_apply("dropout_bits_fwd", dt, x, bits, keep_scale, y, n, stream);
}
extern "C" int vaw_dropout_bits_bwd(vaw_dtype dt, const void* dy, const void* bits, float keep_scale, void* dx, int64_t n, vaw_stream stream) {
    return dropout_bits_apply("dropout_bits_bwd", dt, dy, bits, keep_scale, dx, n, stream);
}

// mode 0: out[b,i,j,:] = in[b,2i,2j,:]  (the even pixels: a stride-2 conv is the stride-1 conv sampled there)
// mode 1: out[b,i,j,:] = (i, j both even) ? in[b,i/2,j/2,:] : 0   (its transpose); out is [B,Ho,Wo,C] in both modes
template <typename T>
__global__ void subsample2_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int Ho, int Wo, int C, int mode) {
    const int64_t n4 = (int64_t)B * Ho * Wo * C / 4;
    const int c4n = C / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int64_t pix = i / c4n;
        const int w = (int)(pix % Wo), h = (int)((pix / Wo) % Ho);
        const int64_t b = pix / ((int64_t)Wo * Ho);
        f32x4 v = {0, 0, 0, 0};
        if (mode == 0) v = load4(in + ((b * 2 * Ho + 2 * h) * (2 * Wo) + 2 * w) * C + 4 * c4);
        else if (!(h & 1) && !(w & 1)) v = load4(in + ((b * (Ho / 2) + h / 2) * (Wo / 2) + w / 2) * C + 4 * c4);
        store4(out + 4 * i, v);
    }
}
extern "C" int vaw_subsample2(vaw_dtype dt, const void* in, void* out, int B, int Ho, int Wo, int C, int mode, vaw_stream stream) {
    VAW_CHECK_ARG(in && out && B > 0 && Ho > 0 && Wo > 0 && C % 4 == 0 && (mode == 0 || (mode == 1 && Ho % 2 == 0 && Wo % 2 == 0)),
                  "subsample2: bad sizes");
    const int64_t n4 = (int64_t)B * Ho * Wo * C / 4;
    BY_DTYPE(dt, (subsample2_kernel<T><<<sgrid(n4, 256), 256, 0, (hipStream_t)stream>>>((const T*)in, (T*)out, B, Ho, Wo, C, mode)));
    VAW_CHECK_LAUNCH("subsample2");
    return VAW_OK;
}

// h[b,p,:] += e[b,:]  (use_scale_shift_norm=False: h + emb_out, reference :250-252); e is f32 with row stride ld
template <typename T>
__global__ void rowvec_add_kernel(T* __restrict__ h, const float* __restrict__ e, int64_t ld, int HW, int C, int64_t n4) {
    const int c4n = C / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int64_t b = i / ((int64_t)c4n * HW);
        store4(h + 4 * i, load4(h + 4 * i) + load4(e + b * ld + 4 * c4));
    }
}
extern "C" int vaw_rowvec_add(vaw_dtype dt, void* h, const float* e, int64_t ld, int B, int HW, int C, vaw_stream stream) {
    VAW_CHECK_ARG(h && e && B > 0 && HW > 0 && C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)e & 15) == 0, "rowvec_add: bad sizes");
    const int64_t n4 = (int64_t)B * HW * C / 4;
    BY_DTYPE(dt, (rowvec_add_kernel<T><<<sgrid(n4, 256), 256, 0, (hipStream_t)stream>>>((T*)h, e, ld, HW, C, n4)));
    VAW_CHECK_LAUNCH("rowvec_add");
    return VAW_OK;
}
// de[b,c] = beta * de[b,c] + sum_p dh[b,p,c]: one workgroup per (sample, 64-channel slab), fixed-order tree
template <typename T>
__global__ void rowvec_sum_kernel(const T* __restrict__ dh, float* __restrict__ de, int64_t ld, int HW, int C, float beta) {
    __shared__ float part[4][64];
    const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), r = threadIdx.x >> 6;
    float acc = 0.f;
    if (c < C)
        for (int p = r; p < HW; p += 4) acc += to_f32(dh[((int64_t)b * HW + p) * C + c]);
    part[r][threadIdx.x & 63] = acc;
    __syncthreads();
    if (r == 0 && c < C) {
        const float t = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        float* o = de + (int64_t)b * ld + c;
        *o = (beta != 0.f ? beta * *o : 0.f) + t;
    }
}
extern "C" int vaw_rowvec_sum(vaw_dtype dt, const void* dh, float* de, int64_t ld, int B, int HW, int C, float beta, vaw_stream stream) {
    VAW_CHECK_ARG(dh && de && B > 0 && HW > 0 && C > 0 && B < 65536, "rowvec_sum: bad sizes");
    dim3 grid(ceil_div(C, 64), B);
    BY_DTYPE(dt, (rowvec_sum_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T*)dh, de, ld, HW, C, beta)));
    VAW_CHECK_LAUNCH("rowvec_sum");
    return VAW_OK;
}

extern "C" int vaw_nchw_to_nhwc(vaw_dtype dt, const float* nchw, void* nhwc, int B, int C, int HW, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && HW > 0, "nchw_to_nhwc: bad sizes");
    const int64_t n = (int64_t)B * C * HW;
    BY_DTYPE(dt, (layout_kernel<T, true><<<sgrid(n, 256), 256, 0, (hipStream_t)stream>>>(nchw, nullptr, nullptr, (T*)nhwc, B, C, HW)));
    VAW_CHECK_LAUNCH("nchw_to_nhwc");
    return VAW_OK;
}
extern "C" int vaw_nhwc_to_nchw(vaw_dtype dt, const void* nhwc, float* nchw, int B, int C, int HW, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && C > 0 && HW > 0, "nhwc_to_nchw: bad sizes");
    const int64_t n = (int64_t)B * C * HW;
    BY_DTYPE(dt, (layout_kernel<T, false><<<sgrid(n, 256), 256, 0, (hipStream_t)stream>>>(nullptr, nchw, (const T*)nhwc, nullptr, B, C, HW)));
    VAW_CHECK_LAUNCH("nhwc_to_nchw");
    return VAW_OK;
}

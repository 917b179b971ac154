// Row-statistics kernels of the DiT block: LayerNorm+adaLN-modulate forward/backward, gated-residual
// backward, and column sums (bias gradients).  All HBM-bound: one wave owns one token row, the row lives
// in registers between the statistics passes (one read of x, one write of the output), reductions are
// wavefront shuffles, and per-sample sums over tokens are combined through LDS in a fixed wave order
// (bitwise reproducible; no float atomics).
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

// The LayerNorm + modulate of ONE token row held in a wave's registers (v[i]: the four columns of slab i of this lane, zero beyond D;
// s: the lane's sum of them, slab by slab).  ln_modulate_fwd_kernel and gate_resid_ln_fwd_kernel both go through these two, so they
// give the same bits on the same row: slab sums per lane, wave_sum, rsqrtf, then (x - mean) * rstd * (1 + scale) + shift.
template <int NV>
__device__ __forceinline__ void ln_row_stats(const f32x4 (&v)[NV], float s, int lane, int D, float eps, float& mean, float& rstd) {
    mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) {
            f32x4 d = v[i] - mean;
            q += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
        }
    }
    rstd = rsqrtf(wave_sum(q) / (float)D + eps);
}
__device__ __forceinline__ f32x4 ln_modulate4(f32x4 v, float mean, float rstd, f32x4 sc, f32x4 sh) {
    f32x4 xh = (v - mean) * rstd;
    return xh * (1.f + sc) + sh;
}
template <typename T, int NV>
__device__ __forceinline__ void ln_row_store(const f32x4 (&v)[NV], float mean, float rstd, const float* __restrict__ sc,
                                             const float* __restrict__ sh, T* __restrict__ orow, int lane, int D) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) store4(orow + c, ln_modulate4(v[i], mean, rstd, load4(sc + c), load4(sh + c)));
    }
}

// NV = number of 256-column slabs a lane walks (D <= 256*NV), D % 4 == 0.
template <typename T, int NV>
__global__ void __launch_bounds__(256)
ln_modulate_fwd_kernel(const float* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale,
                       int64_t mod_ld, T* __restrict__ out, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                       int64_t M, int Tt, int D, float eps, unsigned char* __restrict__ q_out = nullptr,
                       float* __restrict__ q_state = nullptr, int q_e5m2 = 0) {
    const int lane = threadIdx.x & 63;
    // one wave per token row; a wave walks rows blockIdx.x * 4 + wave, + 4 * gridDim.x, ... (the bf16 / f32 launches give every
    // row its own wave; the fp8 launch caps the grid so that each wave folds MANY rows' max |x| into the tensor's running max
    // with one atomic at its end: 32768 waves polling one address cost more than the whole pass -- 104 vs 46 us on DiT-XL/2)
    const float q_inv = q_out ? 1.f / q_state[0] : 1.f;
    float am = 0.f;
    // every launch caps its grid (8 workgroups per CU): a wave walks several rows and requests the NEXT row before it works on the
    // current one -- a row is one 16-byte load per lane and slab, then two wave reductions: with one row per wave (round 3) the
    // only thing in flight during the reductions was other waves' rows, and 4096 three-microsecond workgroups queued behind the
    // dispatcher (3.9-4.2 TB/s of the 6 B/elem).  Row bases are wave-uniform, lanes beyond D re-read column 0 (masked below).
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * 4 + wave, rstep = (int64_t)gridDim.x * 4;
    unsigned colc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const unsigned c = (unsigned)(i * 64 + lane) * 4u;
        colc[i] = c < (unsigned)D ? c : 0u;
    }
    f32x4 nx[NV];
    if (row0 < M) {
#pragma unroll
        for (int i = 0; i < NV; ++i) nx[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + row0 * D + colc[i]));
    }
    for (int64_t row = row0; row < M; row += rstep) {
        const int b = (int)(row / Tt);
        f32x4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[i] = c < D ? nx[i] : f32x4{0, 0, 0, 0};
            s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        }
        if (row + rstep < M) {
#pragma unroll
            for (int i = 0; i < NV; ++i) nx[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + (row + rstep) * D + colc[i]));
        }
        float mean, rstd;
        ln_row_stats<NV>(v, s, lane, D, eps, mean, rstd);
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
        const float* sh = shift + (int64_t)b * mod_ld;
        const float* sc = scale + (int64_t)b * mod_ld;
        if (q_out) {      // fp8 mode: the row goes out as fp8 bytes of its bf16 rounding (the bf16 tensor has no other reader)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < D) {
                    f32x4 xh = (v[i] - mean) * rstd;
                    *reinterpret_cast<unsigned*>(q_out + row * D + c) = fp8_word_of_bf16(xh * (1.f + load4(sc + c)) + load4(sh + c), q_inv, q_e5m2, am);
                }
            }
            continue;
        }
        ln_row_store<T, NV>(v, mean, rstd, sc, sh, out + row * D, lane, D);
    }
    if (q_out) {          // one look at the running max per WORKGROUP (the four waves' maxima meet in LDS)
        __shared__ float wmax[4];
        am = wave_max(am);
        if (lane == 0) wmax[threadIdx.x >> 6] = am;
        __syncthreads();
        if (threadIdx.x < 64) fp8_amax_commit(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])), q_state + 1, lane);
    }
}

// The gated residual add of a DiT branch and the LayerNorm + modulate that reads its result, as one pass over the rows (bf16 mode):
//   x_out = float(y) * gate + x_in          -- what the GEMM's gated-residual epilogue writes from the same y, gate and residual:
//                                             contract != 0: one rounding (gemm_p8_kernel<.., P8_GATE, ..>: v_pk_fma_f32; this file is
//                                             built with contraction off, so the fma is spelled out), else the product rounded first
//                                             (epi_row8 of the other kernels); vaw_gate_resid_fwd_contracts says which
//   out   = (x_out - mean) * rstd * (1 + scale) + shift, mean, rstd     -- ln_row_stats / ln_row_store: the bits of ln_modulate_fwd_kernel
// LN = false: the residual only.  12 bytes per element (8 without the LayerNorm) against 6 + 6 + the 10 of the GEMM epilogue it relieves.
// Streaming as ln_modulate_fwd_kernel: one wave per row, a grid of one resident round, wave-uniform row bases with one clamped column
// offset per lane and slab (no branch around a load), and the NEXT row's y, residual and gate requested before the current row is
// worked on (y and the residual non-temporally: read once).  The sample's (1 + scale) and shift rows (L2) are requested at the top of
// the row, ahead of the next row's loads (loads retire in order) and two wave reductions before their use.
template <int NV, bool LN>
__global__ void __launch_bounds__(256)
gate_resid_ln_fwd_kernel(const bf16_t* __restrict__ y, const float* __restrict__ gate, int64_t gate_ld, const float* __restrict__ x_in,
                         float* __restrict__ x_out, const float* __restrict__ shift, const float* __restrict__ scale, int64_t mod_ld,
                         bf16_t* __restrict__ out, float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t M, int Tt, int D,
                         float eps, int contract) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * 4 + wave, rstep = (int64_t)gridDim.x * 4;
    bool act[NV];
    unsigned col[NV], colc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        col[i] = (unsigned)(i * 64 + lane) * 4u;
        act[i] = col[i] < (unsigned)D;
        colc[i] = act[i] ? col[i] : 0u;
    }
    bf16x4 ny[NV];
    f32x4 nx[NV], ng[NV];
    auto issue = [&](int64_t row) __attribute__((always_inline)) {
        const bf16_t* const y_r = y + row * D;
        const float* const x_r = x_in + row * D;
        const float* const g_r = gate + (row / Tt) * gate_ld;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            ny[i] = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(y_r + colc[i]));
            nx[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x_r + colc[i]));
            ng[i] = load4(g_r + colc[i]);
        }
    };
    if (row0 < M) issue(row0);
    for (int64_t row = row0; row < M; row += rstep) {
        f32x4 scv[LN ? NV : 1], shv[LN ? NV : 1];
        if (LN) {
            const float* const sc = scale + (row / Tt) * mod_ld;
            const float* const sh = shift + (row / Tt) * mod_ld;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                scv[i] = load4(sc + colc[i]);
                shv[i] = load4(sh + colc[i]);
            }
        }
        f32x4 v[NV];
        float s = 0.f;
        if (contract) {       // (uniform) one rounding, the persistent GEMM's epilogue
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const f32x4 r = {__builtin_fmaf((float)ny[i][0], ng[i][0], nx[i][0]), __builtin_fmaf((float)ny[i][1], ng[i][1], nx[i][1]),
                                 __builtin_fmaf((float)ny[i][2], ng[i][2], nx[i][2]), __builtin_fmaf((float)ny[i][3], ng[i][3], nx[i][3])};
                v[i] = act[i] ? r : f32x4{0, 0, 0, 0};
            }
        } else {              // the product rounded first, the row epilogue of the other GEMM kernels (contraction is off in this file)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const f32x4 yf = {(float)ny[i][0], (float)ny[i][1], (float)ny[i][2], (float)ny[i][3]};
                v[i] = act[i] ? yf * ng[i] + nx[i] : f32x4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        if (row + rstep < M) issue(row + rstep);
        float* const xo = x_out + row * D;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (act[i]) __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4*>(xo + col[i]));
        if (LN) {
            float mean, rstd;
            ln_row_stats<NV>(v, s, lane, D, eps, mean, rstd);
            if (lane == 0) {
                mean_out[row] = mean;
                rstd_out[row] = rstd;
            }
            bf16_t* const orow = out + row * D;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                if (act[i]) store4(orow + col[i], ln_modulate4(v[i], mean, rstd, scv[i], shv[i]));
            }
        }
    }
}

// One block per sample; NW waves stride over that sample's T rows.
// FUSE (LayerNorm mode only): the gate backward of the branch that PRECEDES this LayerNorm in the forward pass (its gradient is
// the dres row this kernel has just produced) runs on the row while it is still in registers -- dy = dres * gate, dgate += dres * y,
// column sums of dy -- instead of re-reading dres in a launch of its own (bitwise the same results: same values, same order).
template <typename T, int NV, bool GATE_ONLY, bool QOUT = false, bool FUSE = false>
__global__ void __launch_bounds__((FUSE && NV > 3) ? 512 : 1024)
row_bwd_kernel(const T* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ mean,
               const float* __restrict__ rstd, const float* __restrict__ scale, int64_t mod_ld,
               const float* __restrict__ dres_in, float* __restrict__ dx, float* __restrict__ dshift,
               float* __restrict__ dscale, int64_t dmod_ld, int Tt, int D,
               // GATE_ONLY operands
               const float* __restrict__ dres, const T* __restrict__ y, const float* __restrict__ gate,
               T* __restrict__ dy, float* __restrict__ dgate, float* __restrict__ dy_colpart,
               // gridDim.y > 1: the sample's rows are cut into chunks of rows_per_chunk, one workgroup each; the per-sample
               // column sums then go to part[chunk][b][2][D] and row_bwd_finish_kernel folds the chunks in order
               int rows_per_chunk, float* __restrict__ part,
               // GATE_ONLY, fp8 mode: dy goes out as fp8 bytes of its bf16 rounding instead (q_state: its delayed-scaling state)
               unsigned char* __restrict__ q_out = nullptr, float* __restrict__ q_state = nullptr, int q_e5m2 = 0,
               // LayerNorm mode, optional: the rounding of dx to the act dtype beside it (the GEMM operand a cast pass would make)
               T* __restrict__ dx_act = nullptr) {
    static_assert(!(FUSE && GATE_ONLY), "FUSE extends the LayerNorm mode");
    constexpr int NQ = FUSE ? 4 : 2;                               // per-sample column sums carried
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [NQ][D]
    const float q_inv = ((GATE_ONLY || FUSE) && QOUT) ? 1.f / q_state[0] : 1.f;
    float q_am = 0.f;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int b = blockIdx.x;
    const int t_begin = blockIdx.y * rows_per_chunk;
    const int t_end = t_begin + rows_per_chunk < Tt ? t_begin + rows_per_chunk : Tt;
    f32x4 acc0[NV], acc1[NV], sc[NV];
    f32x4 acc2[FUSE ? NV : 1], acc3[FUSE ? NV : 1];
    // FUSE: four accumulator sets fill the 128 registers a 1024-thread workgroup may use; the sample's (1 + scale) and gate rows
    // then stay in LDS ([NQ][D] sums first, then these two rows) and are re-read per token row
    float* const sc_lds = lds + NQ * D;
    float* const gsc_lds = sc_lds + D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        acc0[i] = f32x4{0, 0, 0, 0};
        acc1[i] = f32x4{0, 0, 0, 0};
        const int c = (i * 64 + lane) * 4;
        const float* src = GATE_ONLY ? gate : scale;
        sc[i] = c < D ? load4(src + (int64_t)b * mod_ld + c) : f32x4{0, 0, 0, 0};
        if (FUSE) {
            acc2[i] = acc3[i] = f32x4{0, 0, 0, 0};
            if (wid == 0 && c < D) {
                store4(sc_lds + c, 1.f + sc[i]);
                store4(gsc_lds + c, load4(gate + (int64_t)b * mod_ld + c));
            }
        }
    }
    if (FUSE) __syncthreads();
    for (int t = t_begin + wid; t < t_end; t += nw) {
        const int64_t row = (int64_t)b * Tt + t;
        if (GATE_ONLY) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < D) {
                    f32x4 g = load4(dres + row * D + c);
                    f32x4 yv = load4(y + row * D + c);
                    f32x4 d = g * sc[i];
                    if (QOUT) *reinterpret_cast<unsigned*>(q_out + row * D + c) = fp8_word_of_bf16(d, q_inv, q_e5m2, q_am);
                    else store4(dy + row * D + c, d);
                    acc0[i] += g * yv;
                    f32x4 dr = {to_f32(from_f32<T>(d[0])), to_f32(from_f32<T>(d[1])), to_f32(from_f32<T>(d[2])), to_f32(from_f32<T>(d[3]))};
                    acc1[i] += dr;                        // sum the values as stored (bf16-rounded in throughput mode)
                }
            }
        } else {
            const float mu = mean[row], rs = rstd[row];
            f32x4 g[NV], xh[NV];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < D) {
                    f32x4 d = load4(dout + row * D + c);
                    xh[i] = (load4(x + row * D + c) - mu) * rs;
                    acc0[i] += d;            // dshift
                    acc1[i] += d * xh[i];    // dscale
                    g[i] = d * (FUSE ? load4(sc_lds + c) : 1.f + sc[i]);
                    s1 += g[i][0] + g[i][1] + g[i][2] + g[i][3];
                    f32x4 gx = g[i] * xh[i];
                    s2 += gx[0] + gx[1] + gx[2] + gx[3];
                } else {
                    g[i] = xh[i] = f32x4{0, 0, 0, 0};
                }
            }
            const float c1 = wave_sum(s1) / (float)D, c2 = wave_sum(s2) / (float)D;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < D) {
                    f32x4 r = (g[i] - c1 - xh[i] * c2) * rs;
                    if (dres_in) r += load4(dres_in + row * D + c);
                    store4(dx + row * D + c, r);
                    if (dx_act) store4(dx_act + row * D + c, r);
                    if (FUSE) {      // the gate backward of vaw_gate_bwd, on the row just produced
                        const f32x4 yv = load4(y + row * D + c);
                        const f32x4 d = r * load4(gsc_lds + c);
                        if (QOUT) *reinterpret_cast<unsigned*>(q_out + row * D + c) = fp8_word_of_bf16(d, q_inv, q_e5m2, q_am);
                        else store4(dy + row * D + c, d);
                        acc2[i] += r * yv;
                        f32x4 dr = {to_f32(from_f32<T>(d[0])), to_f32(from_f32<T>(d[1])), to_f32(from_f32<T>(d[2])), to_f32(from_f32<T>(d[3]))};
                        acc3[i] += dr;
                    }
                }
            }
        }
    }
    if ((GATE_ONLY || FUSE) && QOUT) fp8_amax_commit(q_am, q_state + 1, lane);
    // fixed-order combine of the per-wave column sums
    float* s0 = lds;
    float* s1p = lds + D;
    for (int i = threadIdx.x; i < NQ * D; i += blockDim.x) lds[i] = 0.f;
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
        if (wid == w) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < D) {
                    store4(s0 + c, load4(s0 + c) + acc0[i]);
                    store4(s1p + c, load4(s1p + c) + acc1[i]);
                    if (FUSE) {
                        store4(lds + 2 * D + c, load4(lds + 2 * D + c) + acc2[i]);
                        store4(lds + 3 * D + c, load4(lds + 3 * D + c) + acc3[i]);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (part) {
        float* dst = part + ((int64_t)blockIdx.y * gridDim.x + b) * NQ * D;
        for (int c = threadIdx.x; c < NQ * D; c += blockDim.x) dst[c] = lds[c];
        return;
    }
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        if (GATE_ONLY) {
            dgate[(int64_t)b * dmod_ld + c] = s0[c];
            if (dy_colpart) dy_colpart[(int64_t)b * D + c] = s1p[c];
        } else {
            dshift[(int64_t)b * dmod_ld + c] = s0[c];
            dscale[(int64_t)b * dmod_ld + c] = s1p[c];
            if (FUSE) {
                dgate[(int64_t)b * dmod_ld + c] = lds[2 * D + c];
                if (dy_colpart) dy_colpart[(int64_t)b * D + c] = lds[3 * D + c];
            }
        }
    }
}

// ---- the fused LayerNorm-backward + gate-backward pass for bf16 rows up to 1280 wide (DiT-S / B / L / XL), rebuilt around memory-level
// parallelism (round 4).  row_bwd_kernel<FUSE> above keeps four accumulator sets in registers: at 1024 threads that leaves a wave
// no room to have more than one slab of one row in flight, and the compiler ends every `if (c < D)` block that holds loads with a
// wait for them -- 3.8-4.2 TB/s of its 18 B per element, 89 % of the wave time parked on memory (PMC, round 3).  Here:
//   * 8 waves per workgroup and up to 256 registers each; the four per-sample column sums live in a per-wave LDS slab [4][D]
//     (same additions in the same order as the register version, folded over the waves in wave order at the end);
//   * all four operand rows of a token row (144 bytes per lane) are requested at once, non-temporally, with wave-uniform row
//     bases and one unsigned per-lane column offset (lanes beyond D re-read column 0 and are masked out: no branch around a load);
//   * the NEXT row of the wave is requested before the current one is worked on (two register sets, loop unrolled by two), so a
//     wave always has 144-288 bytes per lane in flight and the two reductions of a row no longer expose a memory latency.
// Arithmetic and its order are those of vaw_ln_modulate_bwd followed by vaw_gate_bwd at 8 waves per workgroup (bitwise: tests).
template <int NV, bool QOUT>
__global__ void __launch_bounds__(512)
row_bwd_fuse8_kernel(const bf16_t* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ mean,
                     const float* __restrict__ rstd, const float* __restrict__ scale, int64_t mod_ld,
                     const float* __restrict__ dres_in, float* __restrict__ dx, float* __restrict__ dshift,
                     float* __restrict__ dscale, int64_t dmod_ld, int Tt, int D, const bf16_t* __restrict__ y,
                     const float* __restrict__ gate, bf16_t* __restrict__ dy, float* __restrict__ dgate, float* __restrict__ dy_colpart,
                     int rows_per_chunk, float* __restrict__ part, unsigned char* __restrict__ q_out, float* __restrict__ q_state,
                     int q_e5m2) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // (1 + scale) row | gate row | [waves][4][D] sums
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int b = blockIdx.x;
    const int t_begin = blockIdx.y * rows_per_chunk;
    const int t_end = t_begin + rows_per_chunk < Tt ? t_begin + rows_per_chunk : Tt;
    float* const sc_lds = lds;
    float* const gsc_lds = lds + D;
    float* const slab = lds + 2 * D + wid * 4 * D;
    const float q_inv = QOUT ? 1.f / q_state[0] : 1.f;
    float q_am = 0.f;
    bool act[NV];
    unsigned col[NV], colc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        col[i] = (unsigned)(i * 64 + lane) * 4u;
        act[i] = col[i] < (unsigned)D;
        colc[i] = act[i] ? col[i] : 0u;
        if (act[i]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) store4(slab + q * D + col[i], f32x4{0, 0, 0, 0});
            if (wid == 0) {
                store4(sc_lds + col[i], 1.f + load4(scale + (int64_t)b * mod_ld + col[i]));
                store4(gsc_lds + col[i], load4(gate + (int64_t)b * mod_ld + col[i]));
            }
        }
    }
    __syncthreads();
    struct RowRegs {
        bf16x4 dq[NV], yq[NV];
        f32x4 xv[NV], rv[NV];
        float mu, rs;
    };
    auto issue = [&](RowRegs& R, int t) __attribute__((always_inline)) {
        const int64_t row = (int64_t)b * Tt + t;
        const bf16_t* const dout_r = dout + row * D;
        const float* const x_r = x + row * D;
        const float* const res_r = dres_in ? dres_in + row * D : x_r;
        const bf16_t* const y_r = y + row * D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            R.dq[i] = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(dout_r + colc[i]));
            R.xv[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x_r + colc[i]));
            R.rv[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(res_r + colc[i]));
            R.yq[i] = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(y_r + colc[i]));
        }
        R.mu = mean[row];
        R.rs = rstd[row];
    };
    auto process = [&](RowRegs& R, int t) __attribute__((always_inline)) {
        const int64_t row = (int64_t)b * Tt + t;
        const float mu = R.mu, rs = R.rs;
        const f32x4 z = {0, 0, 0, 0};
        f32x4 xh[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 d = act[i] ? f32x4{(float)R.dq[i][0], (float)R.dq[i][1], (float)R.dq[i][2], (float)R.dq[i][3]} : z;
            xh[i] = act[i] ? (R.xv[i] - mu) * rs : z;
            const f32x4 g = d * load4(sc_lds + colc[i]);
            s1 += g[0] + g[1] + g[2] + g[3];
            const f32x4 gx = g * xh[i];
            s2 += gx[0] + gx[1] + gx[2] + gx[3];
            if (act[i]) {
                float* p0 = slab + col[i];
                store4(p0, load4(p0) + d);                    // dshift
                store4(p0 + D, load4(p0 + D) + d * xh[i]);    // dscale
            }
        }
        const float c1 = wave_sum(s1) / (float)D, c2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (!act[i]) continue;
            const f32x4 d0 = {(float)R.dq[i][0], (float)R.dq[i][1], (float)R.dq[i][2], (float)R.dq[i][3]};
            const f32x4 g = d0 * load4(sc_lds + col[i]);
            f32x4 r = (g - c1 - xh[i] * c2) * rs;
            if (dres_in) r += R.rv[i];
            __builtin_nontemporal_store(r, reinterpret_cast<f32x4*>(dx + row * D + col[i]));
            const f32x4 yv = {(float)R.yq[i][0], (float)R.yq[i][1], (float)R.yq[i][2], (float)R.yq[i][3]};
            const f32x4 d = r * load4(gsc_lds + col[i]);
            if (QOUT) *reinterpret_cast<unsigned*>(q_out + row * D + col[i]) = fp8_word_of_bf16(d, q_inv, q_e5m2, q_am);
            else store4(dy + row * D + col[i], d);
            const f32x4 dr = {(float)(bf16_t)d[0], (float)(bf16_t)d[1], (float)(bf16_t)d[2], (float)(bf16_t)d[3]};
            float* p2 = slab + 2 * D + col[i];
            store4(p2, load4(p2) + r * yv);                   // dgate
            store4(p2 + D, load4(p2 + D) + dr);               // column sums of dy as stored
        }
    };
    {
        RowRegs A, Bq;
        int t = t_begin + wid;
        if (t < t_end) issue(A, t);
        while (t < t_end) {
            const int t1 = t + nw;
            if (t1 < t_end) issue(Bq, t1);
            process(A, t);
            if (t1 >= t_end) break;
            const int t2 = t1 + nw;
            if (t2 < t_end) issue(A, t2);
            process(Bq, t1);
            t = t2;
        }
    }
    if (QOUT) fp8_amax_commit(q_am, q_state + 1, lane);
    __syncthreads();
    // fold the waves' slabs in wave order (the order of row_bwd_kernel's turn-taking combine)
    for (int idx = threadIdx.x; idx < 4 * D; idx += blockDim.x) {
        const int q = idx / D, c = idx - q * D;
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += lds[2 * D + (w * 4 + q) * D + c];
        if (part) part[((int64_t)blockIdx.y * gridDim.x + b) * 4 * D + idx] = s;
        else if (q == 0) dshift[(int64_t)b * dmod_ld + c] = s;
        else if (q == 1) dscale[(int64_t)b * dmod_ld + c] = s;
        else if (q == 2) dgate[(int64_t)b * dmod_ld + c] = s;
        else if (dy_colpart) dy_colpart[(int64_t)b * D + c] = s;
    }
}
template <int NV, bool QOUT>
static size_t row_fuse8_lds(int D, int block) {
    const size_t lds = (2 + 4 * (size_t)(block / 64)) * (size_t)D * sizeof(float);
    static bool done = false;
    if (!done && lds > 64 * 1024) {
        const hipError_t rc = hipFuncSetAttribute((const void*)row_bwd_fuse8_kernel<NV, QOUT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (rc != hipSuccess) fprintf(stderr, "row_fuse8_lds: hipFuncSetAttribute -> %s\n", hipGetErrorString(rc));
        done = true;
    }
    return lds;
}

// out0[b][c] (row stride ld0) = sum_chunk part[chunk][b][0][c], out1 likewise from [1] (row stride ld1; may be NULL); the fused
// kernel's part rows carry four quantities: out2 / out3 from [2] / [3]
__global__ void row_bwd_finish_kernel(const float* __restrict__ part, int NC, int B, int D, float* __restrict__ out0, int64_t ld0,
                                      float* __restrict__ out1, int64_t ld1, int NQ = 2, float* __restrict__ out2 = nullptr,
                                      int64_t ld2 = 0, float* __restrict__ out3 = nullptr, int64_t ld3 = 0) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * D) return;
    const int b = (int)(i / D), c = (int)(i % D);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int ch = 0; ch < NC; ++ch) {
        const float* src = part + ((int64_t)ch * B + b) * NQ * D;
        a0 += src[c];
        a1 += src[D + c];
        if (NQ == 4) {
            a2 += src[2 * D + c];
            a3 += src[3 * D + c];
        }
    }
    out0[(int64_t)b * ld0 + c] = a0;
    if (out1) out1[(int64_t)b * ld1 + c] = a1;
    if (out2) out2[(int64_t)b * ld2 + c] = a2;
    if (out3) out3[(int64_t)b * ld3 + c] = a3;
}

static int pick_nv(int D) { return (D + 255) / 256; }
// chunks per sample so that small batches still fill the chip: aim at >= target_wgs workgroups, >= 8 rows per chunk.  One rule for
// every backward entry: the fused pass and the pair of kernels it replaces must cut a sample's rows the same way to stay bitwise equal.
// Wide rows (D > 768: the fused pass's four accumulator sets need 176-190 registers) run 512-thread workgroups, two per CU: cut the
// samples into enough chunks for 512 of them (DiT-XL/2 at 128 images: 200 us with 256 workgroups at 3.2 TB/s); narrower rows aim at
// 256 (one per CU; at B >= 256 the single workgroup per sample already streams and the extra fold launch only costs)
static int chunk_target(int nv) { return nv > 3 ? 512 : 256; }
static int pick_chunks(int B, int Tt, bool have_ws, int target_wgs) {
    if (!have_ws) return 1;
    int nc = (target_wgs + B - 1) / B;
    const int max_nc = Tt / 8 > 0 ? Tt / 8 : 1;
    if (nc > max_nc) nc = max_nc;
    return nc < 1 ? 1 : nc;
}
extern "C" int64_t vaw_row_bwd_workspace_floats(int B, int T, int D) { return (int64_t)pick_chunks(B, T, true, 512) * B * 4 * D; }

// (rows up to 1280 wide: 8 waves everywhere, so that the fused pass -- row_bwd_fuse8_kernel -- and the pair of kernels it replaces cut a
// sample's rows into the same per-wave partial sums and stay bitwise equal)
static int row_waves(int nv, int wide_default) { return nv <= 5 ? 8 : wide_default; }
static int pick_block(int Tt, int max_waves = 16) {
    int nw = Tt < max_waves ? Tt : max_waves;
    if (nw < 1) nw = 1;
    return nw * 64;
}
static constexpr size_t kRowLdsMax = 160 * 1024;     // gfx950: LDS per CU, the most one workgroup may ask for

extern "C" int vaw_row_plan(vaw_row_kind kind, vaw_dtype dt, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t base_addr,
                            int64_t workspace_floats, vaw_row_launch* out) {
    VAW_CHECK_ARG(out && kind >= VAW_ROW_LN_FWD && kind <= VAW_ROW_GATE_LN_FWD, "row_plan: bad kind %d", (int)kind);
    vaw_row_launch p = {};
    if (kind == VAW_ROW_GATE_LN_FWD) {
        // the fused gated residual + LayerNorm forward: bf16 rows only, every vector operand on a 16-byte boundary (ldx = the OR of
        // the gate / modulation row strides, base_addr = the OR of the operand addresses); one wave per row as VAW_ROW_LN_FWD
        VAW_CHECK_ARG(dt == VAW_BF16, "gate_resid_ln_modulate_fwd: bf16 rows only (dt=%d)", (int)dt);
        VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && B < (1 << 30) && T < (1 << 30),
                      "gate_resid_ln_modulate_fwd: need D%%4==0, D<=2048 (D=%ld)", (long)D);
        VAW_CHECK_ARG(ldx >= 0 && ldx % 4 == 0, "gate_resid_ln_modulate_fwd: gate_ld and mod_ld must be multiples of 4");
        VAW_CHECK_ARG((base_addr & 15) == 0, "gate_resid_ln_modulate_fwd: every operand must be 16-byte aligned");
        const int nv = pick_nv((int)D);
        const int64_t wgs = (B * T + 3) / 4;
        p.variant = VAW_RV_GATE_LN_FWD;
        p.nv = nv <= 6 ? nv : 8;
        p.nc = 1;
        p.rows_per_chunk = (int)T;
        p.grid_x = (int)(wgs < (1LL << 30) ? wgs : (1LL << 30));
        p.block = 256;
        *out = p;
        return VAW_OK;
    }
    if (kind == VAW_ROW_COLSUM) {
        const int64_t M = B * T, N = D;
        VAW_CHECK_ARG(B > 0 && T > 0 && N > 0 && ldx >= N, "colsum: bad sizes");
        const bool vec = (ldx % 4 == 0) && ((base_addr & 15) == 0);
        const bool wide = dt == VAW_BF16 && N % 8 == 0 && ldx % 8 == 0 && ((base_addr & 15) == 0) && M >= 1024;
        const int64_t rows = wide ? 128 : 512, RB = (M + rows - 1) / rows;
        VAW_CHECK_ARG(RB < 65536 && (N + 255) / 256 < (1LL << 31), "colsum: M too large");
        p.variant = wide ? VAW_RV_COLSUM_BF16X8 : vec ? VAW_RV_COLSUM_VEC4 : VAW_RV_COLSUM_SCALAR;
        p.nc = (int)RB;
        p.rows_per_chunk = (int)rows;
        p.grid_x = (int)((N + 255) / 256);
        p.block = 256;
        p.workspace_floats = RB * N;
        *out = p;
        return VAW_OK;
    }
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && B < (1 << 30) && T < (1 << 30),
                  "row_plan: need D%%4==0, D<=2048 (D=%ld)", (long)D);
    VAW_CHECK_ARG(dt == VAW_F32 || dt == VAW_BF16, "row_plan: dt");
    const int nv = pick_nv((int)D);
    p.nv = nv <= 6 ? nv : 8;
    if (kind == VAW_ROW_LN_FWD || kind == VAW_ROW_LN_FWD_FP8) {
        const int64_t wgs = (B * T + 3) / 4;        // four rows per workgroup, one per wave; the launch caps the grid (see the kernel)
        p.variant = VAW_RV_LN_FWD;
        p.nc = 1;
        p.rows_per_chunk = (int)T;
        p.grid_x = (int)(kind == VAW_ROW_LN_FWD_FP8 ? (wgs < 2048 ? wgs : 2048) : (wgs < (1LL << 30) ? wgs : (1LL << 30)));
        p.block = 256;
        *out = p;
        return VAW_OK;
    }
    const bool fused = kind == VAW_ROW_LN_BWD_GATE || kind == VAW_ROW_LN_BWD_GATE_FP8;
    const int nq = fused ? 4 : 2;           // per-sample column sums carried through the workspace
    int nc = pick_chunks((int)B, (int)T, workspace_floats > 0, chunk_target(nv));
    if (nc > 1 && workspace_floats < (int64_t)nc * B * nq * D) nc = 1;
    p.nc = nc;
    p.rows_per_chunk = (int)((T + nc - 1) / nc);
    p.grid_x = (int)B;
    p.workspace_floats = nc > 1 ? (int64_t)nc * B * nq * D : 0;
    if (!fused) {
        p.variant = kind == VAW_ROW_LN_BWD ? VAW_RV_ROW_BWD : VAW_RV_ROW_GATE;
        p.block = pick_block(p.rows_per_chunk, row_waves(nv, 16));
        p.lds_bytes = 2 * D * (int64_t)sizeof(float);
    } else {
        p.block = pick_block(p.rows_per_chunk, 8);
        // bf16 rows up to 1280 wide: the LDS-slab kernel, while its (1 + scale) and gate rows and one [4][D] slab per wave fit in
        // the CU's LDS (8 waves: D <= 1204).  Otherwise the register-accumulator form: same waves, same row partition, so still
        // bitwise the pair (fewer waves would change the per-wave partial sums).
        const int64_t lds8 = (2 + 4 * (int64_t)(p.block / 64)) * D * (int64_t)sizeof(float);
        const bool bf = kind == VAW_ROW_LN_BWD_GATE_FP8 || dt == VAW_BF16;
        if (bf && nv <= 5 && lds8 <= (int64_t)kRowLdsMax) {
            p.variant = VAW_RV_ROW_FUSE8;
            p.lds_bytes = lds8;
        } else {
            p.variant = VAW_RV_ROW_FUSE;
            p.lds_bytes = 6 * D * (int64_t)sizeof(float);
        }
    }
    *out = p;
    return VAW_OK;
}

#define DISPATCH_NV(nv, CALL)                                       \
    switch (nv) {                                                   \
        case 1: { constexpr int NV = 1; CALL; } break;              \
        case 2: { constexpr int NV = 2; CALL; } break;              \
        case 3: { constexpr int NV = 3; CALL; } break;              \
        case 4: { constexpr int NV = 4; CALL; } break;              \
        case 5: { constexpr int NV = 5; CALL; } break;              \
        case 6: { constexpr int NV = 6; CALL; } break;              \
        default: { constexpr int NV = 8; CALL; } break;             \
    }

#define ROW_PLAN(kind, dt, B, T, D, ldx, base, wsf)                                      \
    vaw_row_launch plan;                                                               \
    {                                                                                  \
        const int rc_ = vaw_row_plan(kind, dt, B, T, D, ldx, base, wsf, &plan);        \
        if (rc_ != VAW_OK) return rc_;                                                 \
    }

extern "C" int vaw_ln_modulate_fwd(vaw_dtype dt, const float* x, const float* shift, const float* scale, int64_t mod_ld,
                                   void* out, float* mean, float* rstd, int B, int T, int D, float eps,
                                   vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0,
                  "ln_modulate_fwd: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    ROW_PLAN(VAW_ROW_LN_FWD, dt, B, T, D, 0, 0, 0);
    const int64_t M = (int64_t)B * T;
    // one resident round of workgroups (what the registers allow per CU x 256 CUs: 7 x 256 for 768-wide bf16 rows -- a grid of
    // 8 per CU left the eighth to a second, nearly empty round), every wave several rows: see the kernel
    static int per_cu[2][9] = {};
    const int nvk = plan.nv, ti = dt == VAW_F32 ? 0 : 1;
    if (!per_cu[ti][nvk]) {
        int nb = 0;
        if (dt == VAW_F32) { DISPATCH_NV(nvk, (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, ln_modulate_fwd_kernel<float, NV>, 256, 0)); }
        else { DISPATCH_NV(nvk, (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, ln_modulate_fwd_kernel<bf16_t, NV>, 256, 0)); }
        per_cu[ti][nvk] = nb > 0 && nb <= 8 ? nb : 8;
    }
    const int64_t cap = 256LL * per_cu[ti][nvk];
    const int grid = (int)(plan.grid_x < cap ? plan.grid_x : cap);
    hipStream_t s = (hipStream_t)stream;
    if (dt == VAW_F32) {
        DISPATCH_NV(nvk, (ln_modulate_fwd_kernel<float, NV><<<grid, plan.block, 0, s>>>(x, shift, scale, mod_ld, (float*)out, mean, rstd, M, T, D, eps)));
    } else {
        DISPATCH_NV(nvk, (ln_modulate_fwd_kernel<bf16_t, NV><<<grid, plan.block, 0, s>>>(x, shift, scale, mod_ld, (bf16_t*)out, mean, rstd, M, T, D, eps)));
    }
    VAW_CHECK_LAUNCH("ln_modulate_fwd");
    return VAW_OK;
}

// fp8 mode: the same forward with the output as fp8 bytes [B*T][D] of the bf16 roundings (delayed scaling: scale in q_state[0],
// running max |x| folded into q_state[1]); bf16 arithmetic path only.
extern "C" int vaw_ln_modulate_fwd_fp8(const float* x, const float* shift, const float* scale, int64_t mod_ld, void* q_out,
                                       float* q_state, vaw_dtype q_format, float* mean, float* rstd, int B, int T, int D, float eps,
                                       vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0 && q_out && q_state,
                  "ln_modulate_fwd_fp8: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    VAW_CHECK_ARG(q_format == VAW_FP8 || q_format == VAW_BF8, "ln_modulate_fwd_fp8: q_format");
    ROW_PLAN(VAW_ROW_LN_FWD_FP8, VAW_BF16, B, T, D, 0, 0, 0);      // grid: 8 workgroups per CU, every wave several rows: see the kernel
    const int64_t M = (int64_t)B * T;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_NV(plan.nv, (ln_modulate_fwd_kernel<bf16_t, NV><<<plan.grid_x, plan.block, 0, s>>>(x, shift, scale, mod_ld, nullptr, mean, rstd, M, T, D, eps,
                                                                                             (unsigned char*)q_out, q_state, q_format == VAW_BF8)));
    VAW_CHECK_LAUNCH("ln_modulate_fwd_fp8");
    return VAW_OK;
}

// The GEMM kernels do not round the gated residual add alike: the persistent kernel's P8_GATE epilogue contracts y * gate + resid to
// one fma, the 64-, 128- and 256-row kernels and the generic one round the product first (their epilogue multiplies and adds behind
// separate run-time switches).  The row pass rounds as the kernel does that vaw_gemm gives the gated launch of the same rows today:
// [B*T, D] = [B*T, D] x [D, D]^T with bias, aux_out, gate and an f32 residual, every operand aligned (proj's launch; fc2's differs in
// K only).  1: one rounding (fma), 0: two.  Host arithmetic (vaw_gemm_plan), follows the process's GEMM knobs like vaw_gemm itself.
extern "C" int vaw_gate_resid_fwd_contracts(int B, int T, int D) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    vaw_epilogue e = {};          // (addresses stand for null-ness and alignment only)
    e.bias = (const float*)0x1000;
    e.aux_out = (void*)0x1000;
    e.gate = (const float*)0x1000;
    e.gate_ld = 6 * (int64_t)D;
    e.resid = (const void*)0x1000;
    e.rows_per_batch = T;
    e.alpha = 1.f;
    e.out_f32 = 1;
    vaw_gemm_launch g;
    const int64_t M = (int64_t)B * T;
    if (vaw_gemm_plan(VAW_BF16, 1, 1, M, D, D, D, D, D, 0x1000, 0x1000, 0x1000, &e, 0, nullptr, &g) != VAW_OK) return 0;
    return g.variant == VAW_GV_PERSISTENT && g.epi_kind == 3 /* P8_GATE (gemm_epi.h) */ && g.split == 1;
}

// x_out = y * gate + x_in and, unless out is NULL, the LayerNorm + modulate of x_out: see gate_resid_ln_fwd_kernel
extern "C" int vaw_gate_resid_ln_modulate_fwd(vaw_dtype dt, const void* y, const float* gate, int64_t gate_ld, const float* x_in,
                                              float* x_out, const float* shift, const float* scale, int64_t mod_ld, void* out,
                                              float* mean, float* rstd, int B, int T, int D, float eps, vaw_stream stream) {
    VAW_CHECK_ARG(y && gate && x_in && x_out && x_in != x_out, "gate_resid_ln_modulate_fwd: y, gate, x_in and a separate x_out are required");
    VAW_CHECK_ARG(!out || (shift && scale && mean && rstd), "gate_resid_ln_modulate_fwd: out needs shift, scale, mean and rstd");
    const uintptr_t addrs = (uintptr_t)y | (uintptr_t)gate | (uintptr_t)x_in | (uintptr_t)x_out |
                            (out ? (uintptr_t)out | (uintptr_t)shift | (uintptr_t)scale : 0);
    ROW_PLAN(VAW_ROW_GATE_LN_FWD, dt, B, T, D, (gate_ld < 0 || mod_ld < 0) ? -1 : (gate_ld | (out ? mod_ld : 0)), (int64_t)(addrs & 15), 0);
    const int64_t M = (int64_t)B * T;
    const int contract = vaw_gate_resid_fwd_contracts(B, T, D);
    // one resident round of workgroups, every wave several rows (as vaw_ln_modulate_fwd)
    static int per_cu[2][9] = {};
    const int nvk = plan.nv, li = out ? 1 : 0;
    if (!per_cu[li][nvk]) {
        int nb = 0;
        if (out) { DISPATCH_NV(nvk, (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gate_resid_ln_fwd_kernel<NV, true>, 256, 0)); }
        else { DISPATCH_NV(nvk, (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gate_resid_ln_fwd_kernel<NV, false>, 256, 0)); }
        per_cu[li][nvk] = nb > 0 && nb <= 8 ? nb : 8;
    }
    const int64_t cap = 256LL * per_cu[li][nvk];
    const int grid = (int)(plan.grid_x < cap ? plan.grid_x : cap);
    hipStream_t s = (hipStream_t)stream;
    if (out) {
        DISPATCH_NV(nvk, (gate_resid_ln_fwd_kernel<NV, true><<<grid, plan.block, 0, s>>>((const bf16_t*)y, gate, gate_ld, x_in, x_out, shift, scale, mod_ld, (bf16_t*)out, mean, rstd, M, T, D, eps, contract)));
    } else {
        DISPATCH_NV(nvk, (gate_resid_ln_fwd_kernel<NV, false><<<grid, plan.block, 0, s>>>((const bf16_t*)y, gate, gate_ld, x_in, x_out, nullptr, nullptr, 0, nullptr, nullptr, nullptr, M, T, D, eps, contract)));
    }
    VAW_CHECK_LAUNCH("gate_resid_ln_modulate_fwd");
    return VAW_OK;
}

// the launch of vaw_ln_modulate_bwd and vaw_ln_modulate_bwd_cast (`who` names the entry point in error messages)
static int ln_modulate_bwd_launch(const char* who, vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                                  const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift, float* dscale,
                                  int64_t dmod_ld, int B, int T, int D, float* workspace, int64_t workspace_floats, void* dx_act,
                                  vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0,
                  "%s: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", who, D);
    ROW_PLAN(VAW_ROW_LN_BWD, dt, B, T, D, 0, 0, workspace ? workspace_floats : 0);
    hipStream_t s = (hipStream_t)stream;
    const int nc = plan.nc, rpc = plan.rows_per_chunk, block = plan.block;
    float* part = nc > 1 ? workspace : nullptr;
    const size_t lds = plan.lds_bytes;
    dim3 grid(B, nc);
    if (dt == VAW_F32) {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<float, NV, false><<<grid, block, lds, s>>>((const float*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rpc, part, nullptr, nullptr, 0, (float*)dx_act)));
    } else {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<bf16_t, NV, false><<<grid, block, lds, s>>>((const bf16_t*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rpc, part, nullptr, nullptr, 0, (bf16_t*)dx_act)));
    }
    if (nc > 1) row_bwd_finish_kernel<<<ceil_div((int64_t)B * D, 256), 256, 0, s>>>(part, nc, B, D, dshift, dmod_ld, dscale, dmod_ld);
    VAW_CHECK_LAUNCH(who);
    return VAW_OK;
}

extern "C" int vaw_ln_modulate_bwd(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                                   const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift,
                                   float* dscale, int64_t dmod_ld, int B, int T, int D, float* workspace,
                                   int64_t workspace_floats, vaw_stream stream) {
    return ln_modulate_bwd_launch("ln_modulate_bwd", dt, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, B, T, D,
                                  workspace, workspace_floats, nullptr, stream);
}

extern "C" int vaw_ln_modulate_bwd_cast(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                                        const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift,
                                        float* dscale, int64_t dmod_ld, int B, int T, int D, float* workspace,
                                        int64_t workspace_floats, void* dx_act, vaw_stream stream) {
    return ln_modulate_bwd_launch("ln_modulate_bwd_cast", dt, dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, B, T,
                                  D, workspace, workspace_floats, dx_act, stream);
}

// vaw_ln_modulate_bwd followed by vaw_gate_bwd of the branch in front of this LayerNorm, as ONE pass (row_bwd_fuse8_kernel for bf16
// rows whose slabs fit in LDS, row_bwd_kernel<FUSE> otherwise): dx = the residual-stream gradient as before; dy_next = dx * gate_next
// (act dtype), dgate_next[b] = sum_t dx * y_next, dy_colsum_partial [B][D] = per-sample sum_t dy_next (as stored).  Bitwise equal to
// the two separate launches wherever those run 8 waves per workgroup too (D <= 1280).
extern "C" int vaw_ln_modulate_bwd_gate(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                                        const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift,
                                        float* dscale, int64_t dmod_ld, const void* y_next, const float* gate_next, void* dy_next,
                                        float* dgate_next, float* dy_colsum_partial, int B, int T, int D, float* workspace,
                                        int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0,
                  "ln_modulate_bwd_gate: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    VAW_CHECK_ARG(y_next && gate_next && dy_next && dgate_next, "ln_modulate_bwd_gate: the gate operands are required");
    ROW_PLAN(VAW_ROW_LN_BWD_GATE, dt, B, T, D, 0, 0, workspace ? workspace_floats : 0);
    hipStream_t s = (hipStream_t)stream;
    const int nc = plan.nc, rpc = plan.rows_per_chunk, block = plan.block;
    float* part = nc > 1 ? workspace : nullptr;
    const size_t lds = plan.lds_bytes;
    dim3 grid(B, nc);
    if (plan.variant == VAW_RV_ROW_FUSE8) {
#define LAUNCH_FUSE8(NVv)                                                                                                              \
    row_bwd_fuse8_kernel<NVv, false><<<grid, block, row_fuse8_lds<NVv, false>(D, block), s>>>(                                          \
        (const bf16_t*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, (const bf16_t*)y_next, gate_next, \
        (bf16_t*)dy_next, dgate_next, dy_colsum_partial, rpc, part, nullptr, nullptr, 0)
        const int nv = plan.nv;
        if (nv == 1) LAUNCH_FUSE8(1); else if (nv == 2) LAUNCH_FUSE8(2); else if (nv == 3) LAUNCH_FUSE8(3); else if (nv == 4) LAUNCH_FUSE8(4); else LAUNCH_FUSE8(5);
    } else if (dt == VAW_F32) {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<float, NV, false, false, true><<<grid, block, lds, s>>>((const float*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, nullptr, (const float*)y_next, gate_next, (float*)dy_next, dgate_next, dy_colsum_partial, rpc, part)));
    } else {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<bf16_t, NV, false, false, true><<<grid, block, lds, s>>>((const bf16_t*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, nullptr, (const bf16_t*)y_next, gate_next, (bf16_t*)dy_next, dgate_next, dy_colsum_partial, rpc, part)));
    }
    if (nc > 1)
        row_bwd_finish_kernel<<<ceil_div((int64_t)B * D, 256), 256, 0, s>>>(part, nc, B, D, dshift, dmod_ld, dscale, dmod_ld, 4, dgate_next, dmod_ld,
                                                                             dy_colsum_partial, D);
    VAW_CHECK_LAUNCH("ln_modulate_bwd_gate");
    return VAW_OK;
}

// fp8 mode: the same fused pass with dy_next as fp8 bytes [B*T][D] of its bf16 roundings (as vaw_gate_bwd_fp8); bf16 arithmetic path.
extern "C" int vaw_ln_modulate_bwd_gate_fp8(const void* dout, const float* x, const float* mean, const float* rstd, const float* scale,
                                            int64_t mod_ld, const float* dres_in, float* dx, float* dshift, float* dscale, int64_t dmod_ld,
                                            const void* y_next, const float* gate_next, void* dy_q, float* q_state, vaw_dtype q_format,
                                            float* dgate_next, float* dy_colsum_partial, int B, int T, int D, float* workspace,
                                            int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0,
                  "ln_modulate_bwd_gate_fp8: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    VAW_CHECK_ARG(y_next && gate_next && dy_q && q_state && dgate_next, "ln_modulate_bwd_gate_fp8: the gate operands are required");
    VAW_CHECK_ARG(q_format == VAW_FP8 || q_format == VAW_BF8, "ln_modulate_bwd_gate_fp8: q_format");
    ROW_PLAN(VAW_ROW_LN_BWD_GATE_FP8, VAW_BF16, B, T, D, 0, 0, workspace ? workspace_floats : 0);
    hipStream_t s = (hipStream_t)stream;
    const int nc = plan.nc, rpc = plan.rows_per_chunk, block = plan.block;
    float* part = nc > 1 ? workspace : nullptr;
    const size_t lds = plan.lds_bytes;
    dim3 grid(B, nc);
    if (plan.variant == VAW_RV_ROW_FUSE8) {
#define LAUNCH_FUSE8Q(NVv)                                                                                                             \
    row_bwd_fuse8_kernel<NVv, true><<<grid, block, row_fuse8_lds<NVv, true>(D, block), s>>>(                                            \
        (const bf16_t*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, (const bf16_t*)y_next, gate_next, \
        nullptr, dgate_next, dy_colsum_partial, rpc, part, (unsigned char*)dy_q, q_state, q_format == VAW_BF8)
        const int nv = plan.nv;
        if (nv == 1) LAUNCH_FUSE8Q(1); else if (nv == 2) LAUNCH_FUSE8Q(2); else if (nv == 3) LAUNCH_FUSE8Q(3); else if (nv == 4) LAUNCH_FUSE8Q(4); else LAUNCH_FUSE8Q(5);
    } else {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<bf16_t, NV, false, true, true><<<grid, block, lds, s>>>((const bf16_t*)dout, x, mean, rstd, scale, mod_ld, dres_in, dx, dshift, dscale, dmod_ld, T, D, nullptr, (const bf16_t*)y_next, gate_next, nullptr, dgate_next, dy_colsum_partial, rpc, part, (unsigned char*)dy_q, q_state, q_format == VAW_BF8)));
    }
    if (nc > 1)
        row_bwd_finish_kernel<<<ceil_div((int64_t)B * D, 256), 256, 0, s>>>(part, nc, B, D, dshift, dmod_ld, dscale, dmod_ld, 4, dgate_next, dmod_ld,
                                                                             dy_colsum_partial, D);
    VAW_CHECK_LAUNCH("ln_modulate_bwd_gate_fp8");
    return VAW_OK;
}

extern "C" int vaw_gate_bwd(vaw_dtype dt, const float* dres, const void* y, const float* gate, int64_t mod_ld, void* dy,
                            float* dgate, int64_t dmod_ld, float* dy_colsum_partial, int B, int T, int D, float* workspace,
                            int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0,
                  "gate_bwd: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    ROW_PLAN(VAW_ROW_GATE_BWD, dt, B, T, D, 0, 0, workspace ? workspace_floats : 0);
    hipStream_t s = (hipStream_t)stream;
    const int nc = plan.nc, rpc = plan.rows_per_chunk, block = plan.block;
    float* part = nc > 1 ? workspace : nullptr;
    const size_t lds = plan.lds_bytes;
    dim3 grid(B, nc);
    if (dt == VAW_F32) {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<float, NV, true><<<grid, block, lds, s>>>(nullptr, nullptr, nullptr, nullptr, nullptr, mod_ld, nullptr, nullptr, nullptr, nullptr, dmod_ld, T, D, dres, (const float*)y, gate, (float*)dy, dgate, dy_colsum_partial, rpc, part)));
    } else {
        DISPATCH_NV(plan.nv, (row_bwd_kernel<bf16_t, NV, true><<<grid, block, lds, s>>>(nullptr, nullptr, nullptr, nullptr, nullptr, mod_ld, nullptr, nullptr, nullptr, nullptr, dmod_ld, T, D, dres, (const bf16_t*)y, gate, (bf16_t*)dy, dgate, dy_colsum_partial, rpc, part)));
    }
    if (nc > 1) row_bwd_finish_kernel<<<ceil_div((int64_t)B * D, 256), 256, 0, s>>>(part, nc, B, D, dgate, dmod_ld, dy_colsum_partial, D);
    VAW_CHECK_LAUNCH("gate_bwd");
    return VAW_OK;
}

// fp8 mode: gate backward with dy as fp8 bytes [B*T][D] of the bf16 roundings (as vaw_ln_modulate_fwd_fp8); y is bf16.
extern "C" int vaw_gate_bwd_fp8(const float* dres, const void* y, const float* gate, int64_t mod_ld, void* dy_q, float* q_state,
                                vaw_dtype q_format, float* dgate, int64_t dmod_ld, float* dy_colsum_partial, int B, int T, int D,
                                float* workspace, int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 4 == 0 && D <= 2048 && mod_ld % 4 == 0 && dy_q && q_state,
                  "gate_bwd_fp8: need D%%4==0, D<=2048, mod_ld%%4==0 (D=%d)", D);
    VAW_CHECK_ARG(q_format == VAW_FP8 || q_format == VAW_BF8, "gate_bwd_fp8: q_format");
    ROW_PLAN(VAW_ROW_GATE_BWD_FP8, VAW_BF16, B, T, D, 0, 0, workspace ? workspace_floats : 0);
    hipStream_t s = (hipStream_t)stream;
    const int nc = plan.nc, rpc = plan.rows_per_chunk, block = plan.block;
    float* part = nc > 1 ? workspace : nullptr;
    const size_t lds = plan.lds_bytes;
    dim3 grid(B, nc);
    DISPATCH_NV(plan.nv, (row_bwd_kernel<bf16_t, NV, true, true><<<grid, block, lds, s>>>(nullptr, nullptr, nullptr, nullptr, nullptr, mod_ld, nullptr, nullptr, nullptr, nullptr, dmod_ld, T, D, dres, (const bf16_t*)y, gate, nullptr, dgate, dy_colsum_partial, rpc, part, (unsigned char*)dy_q, q_state, q_format == VAW_BF8)));
    if (nc > 1) row_bwd_finish_kernel<<<ceil_div((int64_t)B * D, 256), 256, 0, s>>>(part, nc, B, D, dgate, dmod_ld, dy_colsum_partial, D);
    VAW_CHECK_LAUNCH("gate_bwd_fp8");
    return VAW_OK;
}

// ---------------------------------------------------------------------------------------------
// Column sums: out[n] = beta*out[n] + sum_m X[m,n].  Stage 1: 256 columns x 512 rows per block, four row
// groups folded in LDS, one partial row per row-block written to the workspace.  Stage 2: the partial rows
// are added in a fixed order.  No float atomics: bias gradients are bitwise reproducible.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
colsum_partial_kernel(const T* __restrict__ X, int64_t M, int64_t N, int64_t ldx, float* __restrict__ part_out) {
    __shared__ __attribute__((aligned(16))) float part[4][256];
    const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int64_t col = (int64_t)blockIdx.x * 256 + cg * 4;
    const int64_t r0 = (int64_t)blockIdx.y * 512;
    const int64_t r1 = r0 + 512 < M ? r0 + 512 : M;
    f32x4 acc = {0, 0, 0, 0};
    if (col < N) {
        if (col + 4 <= N) {
            for (int64_t r = r0 + rg; r < r1; r += 4) acc += load4(X + r * ldx + col);
        } else {
            for (int64_t r = r0 + rg; r < r1; r += 4)
                for (int j = 0; j < 4 && col + j < N; ++j) acc[j] += to_f32(X[r * ldx + col + j]);
        }
    }
    store4(&part[rg][cg * 4], acc);
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < N)
        part_out[(int64_t)blockIdx.y * N + c] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}
// out[c] = beta*out[c] + sum_r part[r][c], r ascending within each of 32 interleaved row groups, groups folded in
// ascending order: fixed summation tree.  32 columns x 32 row groups per 1024-thread block.
__global__ void __launch_bounds__(1024)
colsum_final_kernel(const float* __restrict__ part, int64_t RB, int64_t N, float* __restrict__ out, float beta) {
    __shared__ float fold[32][33];
    const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int64_t c = (int64_t)blockIdx.x * 32 + cl;
    float acc = 0.f;
    if (c < N)
        for (int64_t r = grp; r < RB; r += 32) acc += part[r * N + c];
    fold[grp][cl] = acc;
    __syncthreads();
    if (grp == 0 && c < N) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 32; ++g) t += fold[g][cl];
        out[c] = (beta != 0.f ? beta * out[c] : 0.f) + t;
    }
}

// bf16, N % 8 == 0, 16-byte aligned rows: 128 rows x 256 columns per workgroup, every lane 16 independent 16-byte loads
// (the 512-row kernel above walks its rows with one dependent 8-byte load at a time: 1.9 TB/s on [16384][2304])
__global__ void __launch_bounds__(256)
colsum_partial_bf16x8_kernel(const bf16_t* __restrict__ X, int64_t M, int64_t N, int64_t ldx, float* __restrict__ part_out) {
    __shared__ __attribute__((aligned(16))) float part[8][256];
    const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int64_t col = (int64_t)blockIdx.x * 256 + cg * 8;
    const int64_t r0 = (int64_t)blockIdx.y * 128;
    f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
    if (col < N) {          // N % 8 == 0: a group of 8 columns is in or out as a whole
        bf16x8 v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t r = r0 + rg + 8 * i;
            v[i] = r < M ? *reinterpret_cast<const bf16x8*>(X + r * ldx + col) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {        // rows ascending: fixed order
            a0 += f32x4{(float)v[i][0], (float)v[i][1], (float)v[i][2], (float)v[i][3]};
            a1 += f32x4{(float)v[i][4], (float)v[i][5], (float)v[i][6], (float)v[i][7]};
        }
    }
    store4(&part[rg][cg * 8], a0);
    store4(&part[rg][cg * 8 + 4], a1);
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < N) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += part[g][threadIdx.x];
        part_out[(int64_t)blockIdx.y * N + c] = t;
    }
}

// any alignment / any N (e.g. the 3-channel output conv): one thread per (row block, column)
template <typename T>
__global__ void colsum_partial_scalar_kernel(const T* __restrict__ X, int64_t M, int64_t N, int64_t ldx, float* __restrict__ part_out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int64_t r0 = (int64_t)blockIdx.y * 512, r1 = r0 + 512 < M ? r0 + 512 : M;
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) acc += to_f32(X[r * ldx + c]);
    part_out[(int64_t)blockIdx.y * N + c] = acc;
}

// Many column-sum folds in ONE launch: job j folds R_j partial rows of N_j columns into out_j exactly as colsum_final_kernel
// would (same summation tree: bitwise the same result).  The bias gradients of all Linear layers of a group of DiT blocks are
// produced as partial rows by the kernels that make dy (gate backward, GELU' epilogue, attention backward) and folded here
// once per group instead of by one 5-microsecond launch each.
struct ReduceJobDev {
    const float* part;
    float* out;
    int64_t R, N;
    int block0, pad_;
};
__global__ void __launch_bounds__(1024)
colsum_final_batched_kernel(const ReduceJobDev* __restrict__ jobs, int n_jobs, float beta) {
    __shared__ float fold[32][33];
    int lo = 0, hi = n_jobs - 1;                      // last job with block0 <= blockIdx.x (uniform: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ReduceJobDev jb = jobs[lo];
    const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int64_t c = (int64_t)(blockIdx.x - jb.block0) * 32 + cl;
    float acc = 0.f;
    if (c < jb.N)
        for (int64_t r = grp; r < jb.R; r += 32) acc += jb.part[r * jb.N + c];
    fold[grp][cl] = acc;
    __syncthreads();
    if (grp == 0 && c < jb.N) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 32; ++g) t += fold[g][cl];
        jb.out[c] = (beta != 0.f ? beta * jb.out[c] : 0.f) + t;
    }
}

extern "C" int64_t vaw_reduce_rows_batched_desc_bytes(int n_jobs) { return (int64_t)n_jobs * (int64_t)sizeof(ReduceJobDev); }

extern "C" int vaw_reduce_rows_batched(int n_jobs, const vaw_reduce_job* jobs, float beta, void* desc_dev, int upload, vaw_stream stream) {
    VAW_CHECK_ARG(n_jobs > 0 && n_jobs <= 4096 && jobs && desc_dev, "reduce_rows_batched: bad arguments");
    static thread_local ReduceJobDev host[4096];
    int64_t blocks = 0;
    for (int j = 0; j < n_jobs; ++j) {
        VAW_CHECK_ARG(jobs[j].partial && jobs[j].out && jobs[j].R > 0 && jobs[j].N > 0, "reduce_rows_batched: job %d", j);
        host[j] = ReduceJobDev{jobs[j].partial, jobs[j].out, jobs[j].R, jobs[j].N, (int)blocks, 0};
        blocks += (jobs[j].N + 31) / 32;
        VAW_CHECK_ARG(blocks < (1 << 30), "reduce_rows_batched: too many columns");
    }
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = vaw_upload_table("reduce_rows_batched", upload, desc_dev, host, sizeof(ReduceJobDev) * n_jobs, s)) return rc;
    colsum_final_batched_kernel<<<(unsigned)blocks, 1024, 0, s>>>((const ReduceJobDev*)desc_dev, n_jobs, beta);
    VAW_CHECK_LAUNCH("reduce_rows_batched");
    return VAW_OK;
}

extern "C" int64_t vaw_colsum_workspace_floats(int64_t M, int64_t N) { return ((M + 127) / 128) * N; }

extern "C" int vaw_reduce_rows(const float* partial, int64_t R, int64_t N, float* out, float beta, vaw_stream stream) {
    VAW_CHECK_ARG(R > 0 && N > 0 && partial && out, "reduce_rows: bad arguments");
    colsum_final_kernel<<<ceil_div(N, 32), 1024, 0, (hipStream_t)stream>>>(partial, R, N, out, beta);
    VAW_CHECK_LAUNCH("reduce_rows");
    return VAW_OK;
}

extern "C" int vaw_colsum(vaw_dtype dt, const void* X, int64_t M, int64_t N, int64_t ldx, float* out, float beta,
                          float* workspace, int64_t workspace_floats, vaw_stream stream) {
    VAW_CHECK_ARG(M > 0 && N > 0 && ldx >= N, "colsum: bad sizes");
    ROW_PLAN(VAW_ROW_COLSUM, dt, M, 1, N, ldx, (int64_t)(uintptr_t)X, workspace_floats);
    const int64_t RB = plan.nc;
    VAW_CHECK_ARG(workspace && workspace_floats >= plan.workspace_floats, "colsum: workspace too small (%ld < %ld floats)",
                  (long)workspace_floats, (long)plan.workspace_floats);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(plan.grid_x, (int)RB);
    if (plan.variant == VAW_RV_COLSUM_BF16X8) {
        colsum_partial_bf16x8_kernel<<<grid, plan.block, 0, s>>>((const bf16_t*)X, M, N, ldx, workspace);
    } else if (plan.variant == VAW_RV_COLSUM_VEC4) {
        if (dt == VAW_F32) colsum_partial_kernel<float><<<grid, plan.block, 0, s>>>((const float*)X, M, N, ldx, workspace);
        else colsum_partial_kernel<bf16_t><<<grid, plan.block, 0, s>>>((const bf16_t*)X, M, N, ldx, workspace);
    } else {
        if (dt == VAW_F32) colsum_partial_scalar_kernel<float><<<grid, plan.block, 0, s>>>((const float*)X, M, N, ldx, workspace);
        else colsum_partial_scalar_kernel<bf16_t><<<grid, plan.block, 0, s>>>((const bf16_t*)X, M, N, ldx, workspace);
    }
    colsum_final_kernel<<<ceil_div(N, 32), 1024, 0, s>>>(workspace, RB, N, out, beta);
    VAW_CHECK_LAUNCH("colsum");
    return VAW_OK;
}

// Multi-head attention softmax(scale * q k^T) v with arbitrary (batch, head, token, channel) strides, so the
// token-major DiT layout (timm Attention) and the channel-major UNet layout (QKVAttention) share kernels.
//
// "rowwise" family (this file, round 1): one wavefront owns one query row (forward, dQ) or one key row
// (dK/dV); lanes run over keys for the score pass and over channels for the value pass, softmax
// statistics are wave shuffles, probabilities cross from the key-indexed to the channel-indexed pass
// through a per-wave LDS row.  Exact f32 arithmetic on f32 or bf16 storage: this is the parity-mode
// kernel and the fallback for shapes the MFMA kernel does not take.  Backward recomputes P from the saved
// row log-sum-exp (no T x T tensor is ever written), and is split in a query-major and a key-major kernel
// so that no gradient needs atomics: results are bitwise reproducible.
#include "common.h"

#define ATT_MAX_TILES 16   // T <= 64*16

struct AttnDev {
    int B, H, T, hd;
    int64_t q_sb, q_sh, q_st, q_sd;
    int64_t o_sb, o_sh, o_st, o_sd;
    float scale;
};

template <typename T>
__device__ __forceinline__ float ldg(const T* p, int64_t off) { return to_f32(p[off]); }

// grid: (ceil(T/4), B*H); block 256 = 4 waves = 4 query rows
template <typename T>
__global__ void __launch_bounds__(256)
attn_fwd_rowwise(AttnDev a, const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ o,
                 float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // per wave: [hd] q row + [T] probabilities
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int i = blockIdx.x * 4 + wid;
    float* qs = lds + wid * (a.hd + a.T);
    float* ps = qs + a.hd;
    const int64_t base = b * a.q_sb + h * a.q_sh;
    if (i < a.T)
        for (int d = lane; d < a.hd; d += 64) qs[d] = ldg(q, base + i * a.q_st + d * a.q_sd);
    __syncthreads();
    if (i >= a.T) return;
    float s[ATT_MAX_TILES];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < ATT_MAX_TILES; ++t) {
        const int j = t * 64 + lane;
        s[t] = -INFINITY;
        if (t * 64 < a.T && j < a.T) {
            float acc = 0.f;
            const int64_t kb = base + j * a.q_st;
            for (int d = 0; d < a.hd; ++d) acc += qs[d] * ldg(k, kb + d * a.q_sd);
            s[t] = acc * a.scale;
            mx = fmaxf(mx, s[t]);
        }
    }
    mx = wave_max(mx);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < ATT_MAX_TILES; ++t) {
        const int j = t * 64 + lane;
        if (t * 64 < a.T && j < a.T) {
            s[t] = __expf(s[t] - mx);
            l += s[t];
        }
    }
    l = wave_sum(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int t = 0; t < ATT_MAX_TILES; ++t) {
        const int j = t * 64 + lane;
        if (t * 64 < a.T && j < a.T) ps[j] = s[t] * inv;
    }
    if (lane == 0) lse[(int64_t)bh * a.T + i] = mx + __logf(l);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int64_t ob = b * a.o_sb + h * a.o_sh + i * a.o_st;
    for (int d = lane; d < a.hd; d += 64) {
        float acc = 0.f;
        const int64_t vb = base + d * a.q_sd;
        for (int j = 0; j < a.T; ++j) acc += ps[j] * ldg(v, vb + j * a.q_st);
        o[ob + d * a.o_sd] = from_f32<T>(acc);
    }
}

// Query-major backward: delta_i, dS row, dQ row.
template <typename T>
__global__ void __launch_bounds__(256)
attn_bwd_q_rowwise(AttnDev a, const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                   const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse,
                   float* __restrict__ delta, T* __restrict__ dq) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // per wave: [hd] q, [hd] dO, [T] dS
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int i = blockIdx.x * 4 + wid;
    float* qs = lds + wid * (2 * a.hd + a.T);
    float* dos = qs + a.hd;
    float* ds = dos + a.hd;
    const int64_t base = b * a.q_sb + h * a.q_sh;
    const int64_t ob = b * a.o_sb + h * a.o_sh + (int64_t)i * a.o_st;
    float dl = 0.f;
    if (i < a.T) {
        for (int d = lane; d < a.hd; d += 64) {
            qs[d] = ldg(q, base + i * a.q_st + d * a.q_sd);
            const float g = ldg(d_o, ob + d * a.o_sd);
            dos[d] = g;
            dl += g * ldg(o, ob + d * a.o_sd);
        }
    }
    __syncthreads();
    if (i >= a.T) return;
    dl = wave_sum(dl);
    const float li = lse[(int64_t)bh * a.T + i];
    if (lane == 0) delta[(int64_t)bh * a.T + i] = dl;
    for (int j = lane; j < a.T; j += 64) {
        float sc = 0.f, dp = 0.f;
        const int64_t kb = base + j * a.q_st;
        for (int d = 0; d < a.hd; ++d) {
            sc += qs[d] * ldg(k, kb + d * a.q_sd);
            dp += dos[d] * ldg(v, kb + d * a.q_sd);
        }
        const float p = __expf(sc * a.scale - li);
        ds[j] = p * (dp - dl);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int d = lane; d < a.hd; d += 64) {
        float acc = 0.f;
        const int64_t kb = base + d * a.q_sd;
        for (int j = 0; j < a.T; ++j) acc += ds[j] * ldg(k, kb + j * a.q_st);
        dq[base + i * a.q_st + d * a.q_sd] = from_f32<T>(acc * a.scale);
    }
}

// Key-major backward: dK row, dV row.
template <typename T>
__global__ void __launch_bounds__(256)
attn_bwd_kv_rowwise(AttnDev a, const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                    const T* __restrict__ d_o, const float* __restrict__ lse, const float* __restrict__ delta,
                    T* __restrict__ dk, T* __restrict__ dv) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // per wave: [hd] k, [hd] v, [T] P, [T] dS
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int j = blockIdx.x * 4 + wid;
    float* ks = lds + wid * (2 * a.hd + 2 * a.T);
    float* vs = ks + a.hd;
    float* ps = vs + a.hd;
    float* ds = ps + a.T;
    const int64_t base = b * a.q_sb + h * a.q_sh;
    const int64_t obase = b * a.o_sb + h * a.o_sh;
    if (j < a.T)
        for (int d = lane; d < a.hd; d += 64) {
            ks[d] = ldg(k, base + j * a.q_st + d * a.q_sd);
            vs[d] = ldg(v, base + j * a.q_st + d * a.q_sd);
        }
    __syncthreads();
    if (j >= a.T) return;
    for (int i = lane; i < a.T; i += 64) {
        float sc = 0.f, dp = 0.f;
        const int64_t qb = base + i * a.q_st, ob = obase + i * a.o_st;
        for (int d = 0; d < a.hd; ++d) {
            sc += ks[d] * ldg(q, qb + d * a.q_sd);
            dp += vs[d] * ldg(d_o, ob + d * a.o_sd);
        }
        const float p = __expf(sc * a.scale - lse[(int64_t)bh * a.T + i]);
        ps[i] = p;
        ds[i] = p * (dp - delta[(int64_t)bh * a.T + i]);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int d = lane; d < a.hd; d += 64) {
        float av = 0.f, ak = 0.f;
        for (int i = 0; i < a.T; ++i) {
            av += ps[i] * ldg(d_o, obase + i * a.o_st + d * a.o_sd);
            ak += ds[i] * ldg(q, base + i * a.q_st + d * a.q_sd);
        }
        dv[base + j * a.q_st + d * a.q_sd] = from_f32<T>(av);
        dk[base + j * a.q_st + d * a.q_sd] = from_f32<T>(ak * a.scale);
    }
}

// bf16 MFMA path (attention_mfma.hip, attention_bwd_big.hip): launchers and the LDS sizes of their images
bool vaw_attn_mfma_ok(vaw_dtype dt, const vaw_attn_desc* d, int64_t q, int64_t k, int64_t v, int64_t o);
int64_t vaw_attn_img_bytes(int hd_image);
int64_t vaw_attn_fwd_big_lds(int hd_image);
int64_t vaw_attn_bwd_big_lds(int hd_image, int nt, int T);
int vaw_attn_fwd_mfma(const vaw_attn_launch& p, const vaw_attn_desc* d, const void* q, const void* k, const void* v, void* o, float* lse,
                      hipStream_t s);
int vaw_attn_bwd_mfma(const vaw_attn_launch& p, const vaw_attn_desc* d, const void* q, const void* k, const void* v, const void* o,
                      const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv, hipStream_t s,
                      float* cs_part = nullptr);
static int g_force_rowwise = 0;
extern "C" void vaw_debug_force_rowwise_attention(int on) { g_force_rowwise = on; }

static int check_desc(const vaw_attn_desc* d, const char* who) {
    VAW_CHECK_ARG(d && d->B > 0 && d->H > 0 && d->T > 0 && d->hd > 0, "%s: bad descriptor", who);
    VAW_CHECK_ARG(d->T <= 64 * ATT_MAX_TILES, "%s: T=%d exceeds %d", who, d->T, 64 * ATT_MAX_TILES);
    VAW_CHECK_ARG((int64_t)d->B * d->H < 65536, "%s: B*H=%ld exceeds grid.y", who, (long)d->B * d->H);
    return VAW_OK;
}
static AttnDev to_dev(const vaw_attn_desc* d) {
    AttnDev a{d->B, d->H, d->T, d->hd, d->q_sb, d->q_sh, d->q_st, d->q_sd, d->o_sb, d->o_sh, d->o_st, d->o_sd, d->scale};
    return a;
}
static int env_switch(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static constexpr int64_t kAttnLdsDefault = 64 * 1024;     // a launch that does not raise its cap with hipFuncSetAttribute

extern "C" int vaw_attn_plan(int dir, vaw_dtype dt, const vaw_attn_desc* d, int64_t q, int64_t k, int64_t v, int64_t o_or_do,
                             int64_t dq, int64_t dk, int64_t dv, vaw_attn_launch* out) {
    VAW_CHECK_ARG(out && dir >= VAW_ATTN_DIR_FWD && dir <= VAW_ATTN_DIR_BWD_COLSUM, "attn_plan: bad direction %d", dir);
    vaw_attn_launch p = {};
    p.status = VAW_ERR_INVALID;
    *out = p;
    const char* who = dir == VAW_ATTN_DIR_FWD ? "attn_fwd" : dir == VAW_ATTN_DIR_BWD ? "attn_bwd" : "attn_bwd_colsum";
    int rc = check_desc(d, who);
    if (rc) return rc;
    VAW_CHECK_ARG(dt == VAW_F32 || dt == VAW_BF16, "%s: dt must be f32 or bf16", who);
    const bool fwd = dir == VAW_ATTN_DIR_FWD;
    const int T = d->T, hd = d->hd;
    p.block = 256;
    p.grid_y = d->B * d->H;
    const bool mfma = !g_force_rowwise && vaw_attn_mfma_ok(dt, d, q, k, v, o_or_do) && (fwd || ((dq | dk | dv) & 7) == 0);
    if (!mfma) {
        // four query (key) rows per workgroup, one per wave, each wave with its rows of f32 in LDS (the cap is not raised)
        p.variant = VAW_AV_ROWWISE;
        p.launches = fwd ? 1 : 2;
        p.grid_x = (T + 3) / 4;
        p.lds_bytes = fwd ? 16 * ((int64_t)hd + T) : 16 * (2 * (int64_t)hd + 2 * T);
        VAW_CHECK_ARG(p.lds_bytes <= kAttnLdsDefault, "%s: the rowwise kernels need %ld bytes of LDS at hd=%d, T=%d (at most %ld)", who,
                      (long)p.lds_bytes, hd, T, (long)kAttnLdsDefault);
        p.status = VAW_OK;
        *out = p;
        return VAW_OK;
    }
    const int img = hd <= 32 ? 32 : hd <= 64 ? 64 : hd <= 96 ? 96 : 128;     // zero-padded head width of the LDS images
    const int64_t ib = vaw_attn_img_bytes(img);
    p.lds_cap_raised = 1;
    p.hd_image = img;
    if (fwd) {
        p.launches = 1;
        // attention_bwd_big.hip: the owner-rows forward.  VAW_ATTN_FWD_BIG 2 (default) = head dims 72 .. 96, 1 = 40 .. 96, 0 = off
        const int big = env_switch("VAW_ATTN_FWD_BIG", 2);
        if (big != 0 && T % 128 == 0 && hd > (big == 1 ? 32 : 64) && hd <= 96) {
            p.variant = VAW_AV_FWD_BIG;
            p.hd_image = hd <= 64 ? 64 : 96;
            p.grid_x = T / 128;
            p.lds_bytes = vaw_attn_fwd_big_lds(p.hd_image);
        } else if (T % 128 == 0 && hd <= 96 && env_switch("VAW_ATTN_QG2", 1) != 0) {
            // two 16-query groups per wave: +10..17 % for head dims <= 64 (tools/attn_bench.py), +30 % for the padded 96-wide images
            // (DiT-XL's 72, UNet_64's 96) now that their rows are conflict-free; 128-wide images keep one group (accumulators)
            p.variant = VAW_AV_FWD_G2;
            p.grid_x = T / 128;
            p.lds_bytes = (img <= 64 ? 6 : 4) * ib;
        } else if (T == 64) {     // a single key block: nothing to double-buffer, keep the LDS footprint (and residency) small
            p.variant = VAW_AV_FWD_T64;
            p.grid_x = 1;
            p.lds_bytes = 3 * ib;
        } else {
            p.variant = VAW_AV_FWD_G1;
            p.grid_x = T / 64;
            p.lds_bytes = (img <= 64 ? 5 : 3) * ib;
        }
        p.status = VAW_OK;
        *out = p;
        return VAW_OK;
    }
    p.launches = 2;
    const int bwd_big = env_switch("VAW_ATTN_BWD_BIG", 2);
    if (T == 64) {        // single block of queries and keys: one fused launch
        p.variant = VAW_AV_BWD_T64;
        p.launches = 1;
        p.grid_x = 1;
        p.lds_bytes = 4 * ib;
        p.colsum_rows = d->B;
    } else if ((bwd_big == 1 || bwd_big == 2) && T % (bwd_big == 2 ? 128 : 256) == 0 && T <= 1024 && hd > 32 && hd <= 96) {
        // attention_bwd_big.hip: VAW_ATTN_BWD_BIG 2 (default) = 32 owner rows per wave (T % 128), 1 = 64 (T % 256), 0 = off
        const int nt = bwd_big == 2 ? 2 : 4, wgr = 64 * nt;
        p.variant = nt == 2 ? VAW_AV_BWD_BIG_NT2 : VAW_AV_BWD_BIG_NT4;
        p.hd_image = hd <= 64 ? 64 : 96;
        p.grid_x = T / wgr;
        p.lds_bytes = vaw_attn_bwd_big_lds(p.hd_image, nt, T);
        p.colsum_rows = (int64_t)d->B * (T / wgr);
    } else if (T % 128 == 0 && hd > 64 && hd <= 96 && env_switch("VAW_ATTN_BWD_G2", 1) != 0) {
        // measured (tools/attn_bench.py, T = 256 / 1024): two groups are +10 % on the 96-wide images with 96 real channels
        // (UNet_64), neutral on DiT-XL's 72-in-96, and 10-20 % SLOWER on 64-wide images, where the third resident workgroup is
        // worth more than the shared fragments: these kernels are occupancy-, not DMA-latency-bound
        p.variant = VAW_AV_BWD_G2;
        p.grid_x = T / 128;
        p.lds_bytes = 6 * ib + 2 * 64 * 4;
        p.colsum_rows = (int64_t)d->B * (T / 128);
    } else {
        p.variant = VAW_AV_BWD_G1;
        p.grid_x = T / 64;
        p.lds_bytes = 4 * ib + 2 * 64 * 4;
        p.colsum_rows = (int64_t)d->B * (T / 64);
    }
    if (dir != VAW_ATTN_DIR_BWD_COLSUM) p.colsum_rows = 0;
    p.status = VAW_OK;
    *out = p;
    return VAW_OK;
}

extern "C" int vaw_attn_fwd(vaw_dtype dt, const vaw_attn_desc* d, const void* q, const void* k, const void* v, void* o,
                            float* lse, vaw_stream stream) {
    vaw_attn_launch p;
    int rc = vaw_attn_plan(VAW_ATTN_DIR_FWD, dt, d, (int64_t)q, (int64_t)k, (int64_t)v, (int64_t)o, 0, 0, 0, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.variant != VAW_AV_ROWWISE) return vaw_attn_fwd_mfma(p, d, q, k, v, o, lse, s);
    AttnDev a = to_dev(d);
    dim3 grid(p.grid_x, p.grid_y);
    const size_t lds = 16 * (size_t)(a.hd + a.T);
    if (dt == VAW_F32)
        attn_fwd_rowwise<float><<<grid, 256, lds, s>>>(a, (const float*)q, (const float*)k, (const float*)v, (float*)o, lse);
    else
        attn_fwd_rowwise<bf16_t><<<grid, 256, lds, s>>>(a, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse);
    VAW_CHECK_LAUNCH("attn_fwd");
    return VAW_OK;
}

static int attn_bwd_go(const vaw_attn_launch& p, vaw_dtype dt, const vaw_attn_desc* d, const void* q, const void* k, const void* v,
                       const void* o, const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv, hipStream_t s,
                       float* cs_part) {
    if (p.variant != VAW_AV_ROWWISE) return vaw_attn_bwd_mfma(p, d, q, k, v, o, d_o, lse, delta, dq, dk, dv, s, cs_part);
    AttnDev a = to_dev(d);
    dim3 grid(p.grid_x, p.grid_y);
    const size_t lds_q = 16 * (size_t)(2 * a.hd + a.T);
    const size_t lds_kv = p.lds_bytes;
    if (dt == VAW_F32) {
        attn_bwd_q_rowwise<float><<<grid, 256, lds_q, s>>>(a, (const float*)q, (const float*)k, (const float*)v, (const float*)o, (const float*)d_o, lse, delta, (float*)dq);
        attn_bwd_kv_rowwise<float><<<grid, 256, lds_kv, s>>>(a, (const float*)q, (const float*)k, (const float*)v, (const float*)d_o, lse, delta, (float*)dk, (float*)dv);
    } else {
        attn_bwd_q_rowwise<bf16_t><<<grid, 256, lds_q, s>>>(a, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)d_o, lse, delta, (bf16_t*)dq);
        attn_bwd_kv_rowwise<bf16_t><<<grid, 256, lds_kv, s>>>(a, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)d_o, lse, delta, (bf16_t*)dk, (bf16_t*)dv);
    }
    VAW_CHECK_LAUNCH("attn_bwd");
    return VAW_OK;
}

extern "C" int vaw_attn_bwd(vaw_dtype dt, const vaw_attn_desc* d, const void* q, const void* k, const void* v,
                            const void* o, const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv,
                            vaw_stream stream) {
    vaw_attn_launch p;
    int rc = vaw_attn_plan(VAW_ATTN_DIR_BWD, dt, d, (int64_t)q, (int64_t)k, (int64_t)v, (int64_t)d_o, (int64_t)dq, (int64_t)dk,
                           (int64_t)dv, &p);
    if (rc) return rc;
    return attn_bwd_go(p, dt, d, q, k, v, o, d_o, lse, delta, dq, dk, dv, (hipStream_t)stream, nullptr);
}

// vaw_attn_bwd that also leaves the column sums of dq | dk | dv behind as partial rows (packed-qkv column order [3][H][hd], the
// bias layout of timm Attention's qkv Linear): colsum_partial [*rows_out][3 H hd] f32, at most B * T / 64 rows.  Only the bf16
// MFMA kernels offer it: VAW_ERR_UNSUPPORTED (nothing launched) otherwise -- call vaw_attn_bwd and vaw_colsum then.
extern "C" int vaw_attn_bwd_colsum(vaw_dtype dt, const vaw_attn_desc* d, const void* q, const void* k, const void* v, const void* o,
                                   const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv,
                                   float* colsum_partial, int64_t* rows_out, vaw_stream stream) {
    vaw_attn_launch p;
    int rc = vaw_attn_plan(VAW_ATTN_DIR_BWD_COLSUM, dt, d, (int64_t)q, (int64_t)k, (int64_t)v, (int64_t)d_o, (int64_t)dq, (int64_t)dk,
                           (int64_t)dv, &p);
    if (rc) return rc;
    VAW_CHECK_ARG(colsum_partial && rows_out, "attn_bwd_colsum: colsum_partial and rows_out are required");
    VAW_CHECK_ARG(*rows_out >= (int64_t)d->B * (d->T / 64 > 0 ? d->T / 64 : 1), "attn_bwd_colsum: *rows_out states a capacity of %ld rows, up to %ld are written",
                  (long)*rows_out, (long)((int64_t)d->B * (d->T / 64 > 0 ? d->T / 64 : 1)));
    if (p.colsum_rows == 0) {
        vaw_set_error("attn_bwd_colsum: only the bf16 MFMA attention kernels carry column sums");
        return VAW_ERR_UNSUPPORTED;
    }
    rc = attn_bwd_go(p, dt, d, q, k, v, o, d_o, lse, delta, dq, dk, dv, (hipStream_t)stream, colsum_partial);
    if (rc == VAW_OK) *rows_out = p.colsum_rows;
    return rc;
}

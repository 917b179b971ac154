// Host side shared by the GEMM translation units: the knobs, the persistent kernel's shape plan, the LDS size of every kernel
// (asserted against the kernels' own configuration where they are defined) and the vaw_epilogue -> EpiDev copy.
// vaw_gemm_plan (gemm_plan.hip) is the one place a launch choice of vaw_gemm is made, vaw_conv3x3_plan (same file) of vaw_conv3x3.
#pragma once
#include "gemm_epi.h"

typedef vaw_gemm_knobs GemmKnobs;
GemmKnobs& vaw_gemm_knobs_state();      // the process's own: environment read once, then vaw_debug_gemm_tile / _force_generic_gemm
int vaw_p8_cus_available();             // CUs a persistent grid may use now (gemm_p8.hip); 256 without a device

// Tile width and split count of the persistent kernel for a shape, or use = false when another kernel should keep it.
struct P8Plan {
    bool use;
    int ntw, split, grid;
};
P8Plan vaw_p8_plan(int64_t M, int64_t N, int64_t K, bool plain_f32, bool want_colsum, int64_t ws_floats, int force, int cus);

// ---- split-K arithmetic shared by vaw_gemm_plan and vaw_conv3x3_plan
// Split-K factor: only for plain f32-output epilogues (the weight gradients: long K = B*T, few output tiles),
// sized so the launch has ~2 workgroups per CU, each split keeping >= 256 of K, within the workspace.
inline int pick_split(int64_t tiles, int64_t K, int64_t MN, int64_t ws_floats, bool plain_f32) {
    if (!plain_f32 || ws_floats <= 0) return 1;
    int64_t s = 512 / tiles;
    if (s > K / 256) s = K / 256;
    if (s > ws_floats / MN) s = ws_floats / MN;
    if (s > 64) s = 64;
    return s < 2 ? 1 : (int)s;
}
inline int no_empty_split(int nk, int split) {
    if (split <= 1) return 1;
    const int per = (nk + split - 1) / split;
    return (nk + per - 1) / per;
}

// split-K launches of gemm_bf16_kernel whose split count divides 8 use its K-range-per-XCD mapping (xcd_parts = 8 / split)
inline int xcd_parts_for(const GemmKnobs& k, int split) { return (k.xcdsplit && (split == 2 || split == 4 || split == 8)) ? 8 / split : 0; }

// dynamic LDS bytes by variant (8 KiB parts of 64 rows x 64 k of bf16; see the kernels)
constexpr int64_t vaw_lds_t128(int bkt) { return (8 * 128 * bkt > 64 * 132 * 4 ? 8 * 128 * bkt : 64 * 132 * 4) + 4 * 128 * 4; }
constexpr int64_t vaw_lds_ring256() { return 4 * 4 * (128 * 32 * 2) + 8 * 256 * 4; }
constexpr int64_t vaw_lds_p8(int ntw) { return 2 * (4 + ntw) * 8192 + 32768; }
constexpr int64_t vaw_lds_sm(int mb, int nb, int stages) { return (int64_t)stages * (mb + nb) * 8192; }
constexpr int64_t vaw_lds_pd(int ntw) { return 3 * (2 + ntw) * 8192 + 8 * 2048; }
constexpr int64_t vaw_lds_ws(int ntw) { return 3 * (2 + ntw) * 8192; }
constexpr int64_t vaw_lds_generic() { return 2 * 16 * 144 * 4; }

// the caller's epilogue as the kernels take it (C, sizes, slab and the partial-sum pointers are the caller's to fill in)
inline EpiDev vaw_epi_dev(const vaw_epilogue* ep, const GemmKnobs& k) {
    EpiDev e{};
    e.alpha = 1.f;
    if (ep) {
        e.bias = ep->bias; e.act = ep->act; e.aux_in = ep->aux_in; e.aux_out = ep->aux_out; e.gate = ep->gate;
        e.gate_ld = ep->gate_ld; e.resid = ep->resid; e.rowadd = ep->rowadd; e.rpb = ep->rows_per_batch;
        e.alpha = ep->alpha; e.beta = ep->beta; e.out_f32 = ep->out_f32; e.resid_act = ep->resid_is_act;
    }
    if (e.rpb <= 0) e.rpb = 1;
    e.debug = k.debug;
    e.direct_epi = k.epi;
    return e;
}

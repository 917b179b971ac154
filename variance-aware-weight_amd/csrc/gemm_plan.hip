// vaw_gemm_plan: every launch choice of vaw_gemm (gemm.hip), as host arithmetic over the call's sizes, alignments and epilogue,
// the knobs and the CU count.  No device call: tests sweep it on the CPU.
#include <stdlib.h>

#include "gemm_plan.h"

extern "C" void vaw_gemm_default_knobs(vaw_gemm_knobs* k) {
    *k = vaw_gemm_knobs{};
    k->tile = -1;
    k->xcdsplit = k->epi = k->nt_aux = 1;
    k->sm_max_m = 8192;
    k->ws_loaders = 4;
    k->cus = 256;
}
GemmKnobs& vaw_gemm_knobs_state() {
    static GemmKnobs state = [] {
        static const struct { const char* env; int GemmKnobs::*field; } kEnv[] = {
            {"VAW_GEMM_BIG", &GemmKnobs::tile}, {"VAW_GEMM_BK", &GemmKnobs::bk}, {"VAW_GEMM_PD", &GemmKnobs::pd}, {"VAW_GEMM_WS", &GemmKnobs::ws},
            {"VAW_GEMM_XCDSPLIT", &GemmKnobs::xcdsplit}, {"VAW_SM_MAX_M", &GemmKnobs::sm_max_m}, {"VAW_SM_WIDE_M", &GemmKnobs::sm_wide_m},
            {"VAW_SM_NB", &GemmKnobs::sm_nb}, {"VAW_SM_STAGES", &GemmKnobs::sm_stages}, {"VAW_WS_LOADERS", &GemmKnobs::ws_loaders},
            {"VAW_GEMM_EPI", &GemmKnobs::epi}, {"VAW_GEMM_DEBUG", &GemmKnobs::debug}, {"VAW_P8_NT", &GemmKnobs::p8_nt}, {"VAW_P8_NT_AUX", &GemmKnobs::nt_aux}};
        GemmKnobs k;
        vaw_gemm_default_knobs(&k);
        for (const auto& e : kEnv)
            if (const char* v = getenv(e.env)) k.*e.field = atoi(v);
        k.ws_loaders = k.ws_loaders == 8 ? 8 : 4;
        k.p8_nt = k.p8_nt == 1;
        k.nt_aux = k.nt_aux != 0;
        k.cus = 0;                        // asked for on every call: vaw_p8_set_reserved_cus moves it
        return k;
    }();
    return state;
}
extern "C" void vaw_debug_force_generic_gemm(int on) { vaw_gemm_knobs_state().force_generic = on; }
extern "C" void vaw_debug_gemm_tile(int mode) { vaw_gemm_knobs_state().tile = mode; }

// the operands can go to an MFMA kernel: any M and N (edge tiles are predicated), as long as rows are whole 16-byte chunks
static bool operands_fast(const GemmKnobs& k, vaw_dtype dt, int64_t M, int64_t N, int64_t K, int64_t A, int64_t lda, int64_t B,
                          int64_t ldb) {
    return dt == VAW_BF16 && !k.force_generic && N % 8 == 0 && K % 64 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ((A | B) & 15) == 0 &&
           M >= 16 && N >= 16;
}
extern "C" int vaw_gemm_uses_bf16_mfma(vaw_dtype dt, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                                       int64_t ldb) {
    return operands_fast(vaw_gemm_knobs_state(), dt, M, N, K, (int64_t)(uintptr_t)A, lda, (int64_t)(uintptr_t)B, ldb) ? 1 : 0;
}

// Shapes where the 256 x 256 kernel is the faster one (tools/gemm_bench.py --tile both: +4..16 % on 4096^3 / 8192^3,
// slower whenever its grid leaves CUs idle or K is short): whole rounds of 256 workgroups, long K, no edge tiles.
static bool big_tile_pays(int64_t M, int64_t N, int64_t K, int64_t n_wg_big) {
    if (M % 256 || N % 256 || K < 2048 || n_wg_big < 256) return false;
    const int64_t rounds = (n_wg_big + 255) / 256;
    return rounds * 256 * 100 <= n_wg_big * 110;      // at most 10 % of the last round idle
}
// Epilogue kind of the persistent kernel (gemm_epi.h): the specialised kernels cover the launches of the training step, P8_ANY the rest
static int p8_epi_kind(const EpiDev& e, bool a_kmajor, bool b_kmajor, int split, bool colsum) {
    const bool bf16_out = !e.out_f32;
    if (split > 1) return P8_SLAB;
    if (e.act == 1 && e.aux_out && !e.gate && !e.resid && !e.rowadd && bf16_out && !colsum) return P8_GELU;
    if (e.act == 2 && !e.bias && !e.aux_out && !e.gate && !e.resid && !e.rowadd && bf16_out && e.alpha == 1.f) return P8_DGELU;
    if (e.act == 0 && e.gate && e.resid && !e.resid_act && e.aux_out && !e.rowadd && e.out_f32 && e.beta == 0.f && !colsum) return P8_GATE;
    if (e.act == 0 && !e.aux_out && !e.gate && !e.resid && !e.rowadd && e.beta == 0.f) return P8_STORE;
    if (a_kmajor && b_kmajor && e.act == 0 && !e.aux_out && !e.gate && e.resid && e.resid_act && !e.rowadd && bf16_out && e.beta == 0.f && !colsum)
        return P8_RESID;           // 1x1 convs with a fused skip add (UNet attention proj_out): P8_ANY ran them at 2.6x the time of the plain store
    return P8_ANY;
}
// Epilogue kind the parked-drain / warp-specialised kernels offer for the launch, or -1.  (Same classification; K-split launches,
// f32 plain outputs, fused row sums and the UNet's residual kinds stay with gemm_p8_kernel.)
static int pd_epi_kind(const EpiDev& e, bool a_kmajor, bool b_kmajor, int64_t M, int64_t N, int64_t K, bool colsum) {
    // (K >= 12 K tiles: the longest drain -- 8 steps + 2 slots of operand lead -- and the two K tiles behind it are unrolled in front of the K loop)
    if (!a_kmajor || K % 64 != 0 || K / 64 < 12 || N % 8 != 0 || M < 128) return -1;
    const bool bf16_out = !e.out_f32;
    if (e.act == 1 && e.aux_out && !e.gate && !e.resid && !e.rowadd && bf16_out && !colsum && b_kmajor) return P8_GELU;
    if (e.act == 2 && !e.bias && !e.aux_out && !e.gate && !e.resid && !e.rowadd && bf16_out && e.alpha == 1.f && !b_kmajor) return P8_DGELU;
    if (e.act == 0 && e.gate && e.resid && !e.resid_act && e.aux_out && !e.rowadd && e.out_f32 && e.beta == 0.f && !colsum && b_kmajor &&
        e.rpb % 8 == 0)
        return P8_GATE;
    if (e.act == 0 && !e.aux_out && !e.gate && !e.resid && !e.rowadd && e.beta == 0.f && bf16_out) return P8_STORE;
    return -1;
}
// their tile width: the one with fewer rounds of workgroups; a 192-column item costs ~0.8 of a 256-column one
static int pd_pick_ntw(int64_t M, int64_t N, int cus) {
    double best = 1e30;
    int ntw = 4;
    for (int t = 4; t >= 3; --t) {
        const int bn = 64 * t;
        if (t == 3 && ((N + 191) / 192) * 192 > ((N + 255) / 256) * 256) continue;
        const int64_t items = ((M + 127) / 128) * ((N + bn - 1) / bn);
        const double c = (double)((items + cus - 1) / cus) * (t == 4 ? 1.0 : 0.8);
        if (c < best - 1e-9) { best = c; ntw = t; }
    }
    return ntw;
}

// The kernel and its tile parameters for a launch the MFMA kernels can take, in the order of preference: small-M ring, parked-drain /
// warp-specialised, persistent, 256 x 256 ring, 128 x 128.  Fills variant .. lds_bytes, colsum_rows and rowsum_mode.
static int plan_mfma(vaw_gemm_launch& p, const GemmKnobs& k, const EpiDev& e, bool a_kmajor, bool b_kmajor, int64_t M, int64_t N, int64_t K,
                     int64_t ldc, int64_t C, int64_t ws, bool colsum, bool cs_part, bool rowsum, bool plain_f32) {
    const int t = k.tile;
    const int64_t rows64 = (M + 63) / 64;
    const bool cs_room64 = !colsum || cs_part || ws >= rows64 * N;      // the 64-row kernels fold twice the rows of the 128-row ones
    p.block = 256;
    p.bkt = 64;
    // small M (strong-scaling batches: a few thousand token rows): 64-row tiles with a deep LDS-DMA ring (gemm_sm.hip).  Measured
    // (tools/gemm_bench.py --tile sm, DiT-B/4 shapes): it wins on every 768-wide layer up to 4096 rows, and up to 8192 rows on those
    // with K = 768 (proj: 33.2 -> 24.4 us) and on fc2's forward (K = 3072: 72.7 -> 61.2); the wide layers (N >= 2304) tie at 2048 rows
    // and lose above, and the long-K launches (adaLN's input gradient) keep their split-K path (161 us here against 40 + 38 split)
    const bool sm_few_tiles = N <= 1024 && K <= 4096 && (M <= 4096 || (M <= 8192 && (K <= 1024 || b_kmajor)));
    // wide layers at small M (fc1, fc2's GELU' input gradient, qkv at 2048-4096 rows): 128 x 128 tiles on the same ring
    const bool sm_wide = !sm_few_tiles && M <= k.sm_wide_m && K <= 4096 && ((M + 127) / 128) * ((N + 127) / 128) <= 1024;
    const bool sm_forced = t >= 5 && t <= 8;
    if (a_kmajor && ((M <= k.sm_max_m && (sm_few_tiles || sm_wide) && t < 0) || sm_forced) && !rowsum && cs_room64) {
        // 64 x 128 tiles when they still give every CU a workgroup, else 64 x 64; 3 stages (2-3 workgroups per CU) for multi-round launches
        p.variant = VAW_GV_SMALL_M;
        p.mb = t == 8 ? 2 : (t >= 5 ? 1 : (sm_wide && !sm_few_tiles) ? 2 : 1);
        p.nb = p.mb == 2 ? 2 : t == 6 ? 1 : t == 7 ? 2 : k.sm_nb ? (k.sm_nb == 1 ? 1 : 2) : ((M >= 4096 && K >= 2048) ? 2 : 1);
        const int64_t rows_t = (M + 64 * p.mb - 1) / (64 * p.mb), tiles = rows_t * ((N + 64 * p.nb - 1) / (64 * p.nb));
        VAW_CHECK_ARG(tiles < (1LL << 31), "gemm: grid too large");
        p.stages = k.sm_stages ? (k.sm_stages == 3 ? 3 : 4) : (tiles > 256 ? 3 : 4);
        p.grid_x = (int)tiles;
        p.lds_bytes = vaw_lds_sm(p.mb, p.nb, p.stages);
        p.colsum_rows = rows_t;
        return VAW_OK;
    }
    const int64_t n_wg = ((M + 127) / 128) * ((N + 127) / 128);
    VAW_CHECK_ARG(n_wg < (1LL << 31), "gemm: grid too large");
    const bool fused_rowsum = rowsum && !a_kmajor && !colsum;     // row sums of A ride on the 128 x 128 kernel
    const bool plain_bf16 = !e.out_f32 && !e.bias && !e.act && !e.aux_out && !e.gate && !e.resid && !e.rowadd && e.beta == 0.f &&
                            N % 4 == 0 && ldc % 4 == 0 && (C & 7) == 0;
    p.rowsum_mode = fused_rowsum ? VAW_GS_FUSED : rowsum ? VAW_GS_SEPARATE : VAW_GS_NONE;
    // parked-drain / warp-specialised kernels: the un-split launches of the Linear layers whose epilogue they can hide under the next
    // tile's K loop.  Measured level with or behind the 256-row kernel, so by shape only under VAW_GEMM_PD / _WS
    const bool ws_forced = t >= 12 && t <= 14, pd_forced = (t >= 9 && t <= 11) || ws_forced;
    const int pd_kind = (pd_forced || ((k.pd || k.ws) && t == -1)) && k.bk == 0 && !rowsum && cs_room64
                            ? pd_epi_kind(e, a_kmajor, b_kmajor, M, N, K, colsum) : -1;
    if (pd_kind >= 0) {
        const int ntw = (t == 10 || t == 13) ? 4 : (t == 11 || t == 14) ? 3 : pd_pick_ntw(M, N, k.cus);
        const int64_t items = ((M + 127) / 128) * ((N + 64 * ntw - 1) / (64 * ntw));
        // by shape: at least two rounds of workgroups (a workgroup's last epilogue leaves in the open), K of the blocks' Linear layers
        if (pd_forced || (items >= 2 * k.cus && K >= 768 && K <= 4096)) {
            const bool wsk = ws_forced || (k.ws && !pd_forced);
            p.variant = wsk ? VAW_GV_WARP_SPEC : VAW_GV_PARKED_DRAIN;
            p.ntw = ntw;
            p.epi_kind = pd_kind;
            p.grid_x = (int)(items < k.cus ? items : k.cus);
            p.block = wsk ? 512 + 64 * ((ntw == 3 && k.ws_loaders == 8) ? 8 : 4) : 512;      // (the kernel has 4 or 8 loader waves)
            p.lds_bytes = wsk ? vaw_lds_ws(ntw) : vaw_lds_pd(ntw);
            p.colsum_rows = rows64;
            return VAW_OK;
        }
    }
    {
        const int force = t == -1 ? -1 : t == 4 ? 1 : (t == 2 || t == 3) ? t : 0;
        const bool p8_epi_ok = !(e.act == 2 && e.gate) && !(e.resid && e.rowadd);     // gemm_epi.h: EpiOps has two slots
        const P8Plan pl = (k.bk == 0 && !fused_rowsum && p8_epi_ok)
                              ? vaw_p8_plan(M, N, K, plain_f32 || (plain_bf16 && !rowsum && K >= 2048 && ws > 0), colsum, ws, force, k.cus)
                              : P8Plan{false, 4, 1, 0};
        // small M: a persistent launch that gives only half the CUs an item loses to the 128 x 128 kernel (fc1 at 2048 rows: 28.7 vs 22.0 us)
        const bool p8_half_empty = force < 0 && M <= 4096 && pl.use && pl.grid < 200 &&
                                   ((M + 255) / 256) * ((N + 64 * pl.ntw - 1) / (64 * pl.ntw)) * pl.split < 200;
        if (pl.use && !p8_half_empty) {
            p.variant = VAW_GV_PERSISTENT;
            p.ntw = pl.ntw;
            p.split = pl.split;
            p.epi_kind = p8_epi_kind(e, a_kmajor, b_kmajor, pl.split, colsum);
            p.grid_x = pl.grid;
            p.block = 512;
            p.lds_bytes = vaw_lds_p8(pl.ntw);
            p.colsum_rows = (M + 127) / 128;
            return VAW_OK;
        }
    }
    const int64_t n_wgb = ((M + 255) / 256) * ((N + 255) / 256);
    if (k.bk == 0 && !fused_rowsum && (t == 1 || (t == -1 && big_tile_pays(M, N, K, n_wgb)))) {
        p.variant = VAW_GV_RING256;
        p.bkt = 32;
        p.split = no_empty_split((int)(K / 32), colsum ? 1 : pick_split(n_wgb * 2, K, M * N, ws, plain_f32));
        p.grid_x = (int)n_wgb;
        p.grid_y = p.split;
        p.block = 512;
        p.lds_bytes = vaw_lds_ring256();
        p.colsum_rows = (M + 255) / 256;
        return VAW_OK;
    }
    // 128 x 128.  Stage depth 32 (3 workgroups per CU) for the K <= 4096 input-gradient launches with at least ~3 tiles per CU to
    // overlap its K steps (measured: 768 tiles at batch 256); with fewer every K step is exposed latency and 64 halves their number
    p.bkt = k.bk == 32 || k.bk == 64 ? k.bk : ((a_kmajor && !b_kmajor && K <= 4096 && n_wg >= 3 * 256) ? 32 : 64);
    p.variant = p.bkt == 32 ? VAW_GV_T128_BK32 : VAW_GV_T128_BK64;
    int split = colsum ? 1 : pick_split(n_wg, K, M * N, ws - (fused_rowsum ? 64 * M : 0), plain_f32);
    // small-M input gradients (96-192 tiles, long K): a plain bf16 result is K-split too (f32 slabs, the reduce writes bf16)
    if (split == 1 && plain_bf16 && !colsum && !rowsum && ws > 0 && K >= 2048 && n_wg <= 256) {
        int64_t sp = 512 / n_wg;
        if (sp > K / 512) sp = K / 512;
        if (sp > ws / (M * N)) sp = ws / (M * N);
        if (sp > 8) sp = 8;
        if (sp >= 2) split = (int)sp;
    }
    p.split = no_empty_split((int)(K / p.bkt), split);
    p.xcd_parts = xcd_parts_for(k, p.split);
    p.grid_x = p.xcd_parts ? (int)(8 * ((n_wg + p.xcd_parts - 1) / p.xcd_parts)) : (int)n_wg;
    p.grid_y = p.xcd_parts ? 1 : p.split;
    p.lds_bytes = vaw_lds_t128(p.bkt);
    p.colsum_rows = (M + 127) / 128;
    return VAW_OK;
}

// a vaw_colsum pass over an [R][Ncols] matrix (rowsum_a_out off the fused path; column sums of the generic kernel): its two launches,
// and its workspace, which it reuses after the GEMM's own
static int colsum_pass(vaw_gemm_launch& p, vaw_dtype dt, int64_t R, int64_t Ncols, int64_t ld, int64_t addr, int64_t ws) {
    vaw_row_launch rp;
    const int rc = vaw_row_plan(VAW_ROW_COLSUM, dt, R, 1, Ncols, ld, addr, ws, &rp);
    if (rc) return rc;
    if (rp.workspace_floats > p.workspace_floats_used) p.workspace_floats_used = rp.workspace_floats;
    p.launches += 2;
    return VAW_OK;
}

extern "C" int vaw_gemm_plan(vaw_dtype dt, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                             int64_t ldc, int64_t A, int64_t B, int64_t C, const vaw_epilogue* ep, int64_t ws,
                             const vaw_gemm_knobs* knobs, vaw_gemm_launch* out) {
    VAW_CHECK_ARG(out, "gemm_plan: out is NULL");
    vaw_gemm_launch p = {};
    p.status = VAW_ERR_INVALID;
    p.epi_kind = -1;
    p.split = p.grid_y = p.grid_z = 1;
    *out = p;
    GemmKnobs k = knobs ? *knobs : vaw_gemm_knobs_state();
    if (k.cus <= 0) k.cus = vaw_p8_cus_available();
    if (ws < 0) ws = 0;
    VAW_CHECK_ARG(M > 0 && N > 0 && K > 0 && A && B && C, "gemm: bad sizes M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
    VAW_CHECK_ARG(M < (1LL << 31) && N < (1LL << 31), "gemm: M, N must fit 31 bits");
    VAW_CHECK_ARG(lda >= (a_kmajor ? K : M) && ldb >= (b_kmajor ? K : N) && ldc >= N, "gemm: leading dimension too small");
    EpiDev e = vaw_epi_dev(ep, k);
    const bool cs_final = ep && ep->colsum_out, cs_part = ep && ep->colsum_partial_out;      // deferred fold: partial rows stay with the caller
    VAW_CHECK_ARG(!cs_part || (!cs_final && ep->colsum_rows_out), "gemm: colsum_partial_out excludes colsum_out and needs colsum_rows_out");
    const bool colsum = cs_final || cs_part, rowsum = ep && ep->rowsum_a_out;
    VAW_CHECK_ARG(!rowsum || ws >= 64 * M, "gemm: rowsum_a_out needs a workspace");
    VAW_CHECK_ARG(e.act >= 0 && e.act <= 2, "gemm: unknown act %d", e.act);
    VAW_CHECK_ARG(e.act != 2 || e.aux_in, "gemm: act=2 needs aux_in");
    VAW_CHECK_ARG(!(e.gate || e.rowadd) || ep->rows_per_batch > 0, "gemm: gate/rowadd need rows_per_batch");
    VAW_CHECK_ARG(e.beta == 0.f || e.out_f32 || dt == VAW_F32, "gemm: beta needs f32 output");
    if (dt == VAW_F32) e.out_f32 = 1;
    const bool plain_f32 = e.out_f32 && !e.bias && !e.act && !e.aux_out && !e.gate && !e.resid && !e.rowadd && N % 4 == 0 &&
                           ldc % 4 == 0 && (C & 15) == 0;
    // the vector epilogue of the MFMA kernels needs every epilogue operand 16-byte aligned
    const bool epi_aligned = ldc % 8 == 0 && e.gate_ld % 4 == 0 &&
                             (((C | (int64_t)(uintptr_t)e.bias | (int64_t)(uintptr_t)e.aux_in | (int64_t)(uintptr_t)e.aux_out |
                                (int64_t)(uintptr_t)e.gate | (int64_t)(uintptr_t)e.resid | (int64_t)(uintptr_t)e.rowadd) & 15) == 0);
    VAW_CHECK_ARG(!cs_final || ws >= ((M + 127) / 128) * N, "gemm: colsum_out needs a workspace of max(ceil(M/128), ceil(M/512))*N floats");
    p.launches = 1;
    int rc;
    if (operands_fast(k, dt, M, N, K, A, lda, B, ldb) && epi_aligned && (a_kmajor || M % 8 == 0)) {
        if ((rc = plan_mfma(p, k, e, a_kmajor != 0, b_kmajor != 0, M, N, K, ldc, C, ws, colsum, cs_part, rowsum, plain_f32)) != VAW_OK) return rc;
        p.colsum_mode = !colsum ? VAW_GC_NONE : cs_part ? VAW_GC_DEFERRED : VAW_GC_FOLD;
        if (!colsum) p.colsum_rows = 0;
    } else {
        // generic kernel: exact f32, any shape; column sums as a pass over the output just written (one complete row as the only
        // "partial" row of a deferred fold)
        p.variant = VAW_GV_GENERIC;
        p.bkt = 16;
        const int64_t tiles = (int64_t)ceil_div(N, 128) * ceil_div(M, 128);
        int split = colsum ? 1 : pick_split(tiles, K, M * N, ws, plain_f32);
        if (split > 1) {
            const int64_t kchunk = ((K + split - 1) / split + 15) / 16 * 16;
            split = (int)((K + kchunk - 1) / kchunk);
        }
        p.split = p.grid_z = split;
        p.grid_x = ceil_div(N, 128);
        p.grid_y = ceil_div(M, 128);
        p.block = 256;
        p.lds_bytes = vaw_lds_generic();
        p.rowsum_mode = rowsum ? VAW_GS_SEPARATE : VAW_GS_NONE;
        p.colsum_mode = colsum ? VAW_GC_SEPARATE : VAW_GC_NONE;
        p.colsum_rows = colsum ? 1 : 0;
    }
    const bool fused = p.rowsum_mode == VAW_GS_FUSED;
    p.reduce = p.split == 1 ? VAW_GR_NONE : !e.out_f32 ? VAW_GR_BF16 : fused ? VAW_GR_F32_ROWSUM : VAW_GR_F32;
    p.workspace_floats_used = (p.split > 1 ? (int64_t)p.split * M * N : 0) + (fused ? (int64_t)p.split * M : 0) +
                              (p.colsum_mode == VAW_GC_FOLD ? p.colsum_rows * N : 0);
    p.launches += (p.reduce != VAW_GR_NONE) + (fused && p.split == 1) + (p.colsum_mode == VAW_GC_FOLD);
    // A stored [K][M] (a_kmajor = 0): its row sums are a column sum over its K rows
    if (p.rowsum_mode == VAW_GS_SEPARATE && !a_kmajor && (rc = colsum_pass(p, dt, K, M, lda, A, ws)) != VAW_OK) return rc;
    if (p.colsum_mode == VAW_GC_SEPARATE && (rc = colsum_pass(p, e.out_f32 ? VAW_F32 : dt, M, N, ldc, C, ws)) != VAW_OK) return rc;
    *out = p;       // the launch as chosen; status stays VAW_ERR_INVALID for the refusals below
    VAW_CHECK_ARG(!cs_part || p.colsum_rows <= *ep->colsum_rows_out, "gemm: colsum_partial_out holds %ld rows, this launch writes %ld",
                  (long)*ep->colsum_rows_out, (long)p.colsum_rows);
    VAW_CHECK_ARG(p.rowsum_mode != VAW_GS_SEPARATE || !a_kmajor, "gemm: rowsum_a_out is defined for a_kmajor = 0 (weight-gradient layout) only");
    VAW_CHECK_ARG(p.workspace_floats_used <= ws, "gemm: this launch needs a workspace of %ld floats, it has %ld", (long)p.workspace_floats_used,
                  (long)ws);
    out->status = p.status = VAW_OK;
    return VAW_OK;
}

// vaw_conv3x3_plan: every check and launch choice of vaw_conv3x3 (gemm.hip) and of the persistent kernel's conv entry
// (gemm_p8_conv.hip).  Invalid arguments first, then the shapes the explicit path must take, then the kernel.
extern "C" int vaw_conv3x3_plan(vaw_dtype dt, int mode, int64_t act, int64_t act2, int64_t w, int64_t out, int B, int H, int W, int Ci,
                                int Co, const vaw_epilogue* ep, int64_t workspace, int64_t ws, const vaw_gemm_knobs* knobs, int cus,
                                vaw_conv3x3_launch* plan) {
    VAW_CHECK_ARG(plan, "conv3x3_plan: plan is NULL");
    vaw_conv3x3_launch p = {};
    p.status = VAW_ERR_INVALID;
    p.epi_kind = -1;
    p.split = p.grid_y = 1;
    *plan = p;
    const GemmKnobs& k = knobs ? *knobs : vaw_gemm_knobs_state();
    if (cus <= 0) cus = k.cus > 0 ? k.cus : vaw_p8_cus_available();
    if (!workspace || ws < 0) ws = 0;
    VAW_CHECK_ARG(mode >= 0 && mode <= 2 && act && (w || mode == 2) && out && B > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0,
                  "conv3x3: bad arguments");
    EpiDev e = vaw_epi_dev(ep, k);
    if (mode == 2) e.out_f32 = 1;
    const bool colsum = ep && ep->colsum_out, bias_grad = ep && ep->rowsum_a_out;
    VAW_CHECK_ARG(!bias_grad || mode == 2, "conv3x3: rowsum_a_out (bias gradient) belongs to mode 2");
    VAW_CHECK_ARG(!(colsum && mode == 2), "conv3x3: mode 2 takes rowsum_a_out, not colsum_out");
    // ---- shapes of the explicit path: nothing is launched
    const auto unsupported = [&] { plan->status = VAW_ERR_UNSUPPORTED; return VAW_ERR_UNSUPPORTED; };
    if (dt != VAW_BF16 || k.force_generic) return unsupported();
    const int64_t Mpix = (int64_t)B * H * W;
    int64_t M, N, K;           // the 128 x 128 kernel's problem
    if (mode == 0) { M = Mpix; N = Co; K = 9LL * Ci; if (Ci % 64) return unsupported(); }
    else if (mode == 1) { M = Mpix; N = Ci; K = 9LL * Co; if (Co % 64) return unsupported(); }
    else { M = Co; N = 9LL * Ci; K = Mpix; if (Ci % 8 || Mpix % 64 || Co % 8 || !act2) return unsupported(); }
    if (N % 8 || M < 16 || N < 16 || Mpix >= (1LL << 31)) return unsupported();
    if (((act | act2 | w | out) & 15) != 0) return unsupported();
    VAW_CHECK_ARG(e.beta == 0.f || e.out_f32, "conv3x3: beta needs f32 output");
    const bool epi_aligned = e.gate_ld % 4 == 0 && ((((uintptr_t)e.bias | (uintptr_t)e.aux_in | (uintptr_t)e.aux_out | (uintptr_t)e.gate |
                                                     (uintptr_t)e.resid | (uintptr_t)e.rowadd) & 15) == 0);
    if (!epi_aligned) return unsupported();
    VAW_CHECK_ARG(!colsum || ws >= ((M + 127) / 128) * N, "conv3x3: colsum_out needs a workspace");
    p.launches = 1;
    // ---- the persistent 256-row kernel first; mode 2 runs the transposed problem dW^T [9 Ci][Co] there, always K-split
    const int force = k.tile == -1 ? -1 : k.tile == 4 ? 1 : (k.tile == 2 || k.tile == 3) ? k.tile : 0;
    const int64_t M8 = mode == 2 ? N : M, N8 = mode == 2 ? M : N;
    bool p8 = !colsum && force != 0 && Mpix * (Ci > Co ? Ci : Co) < (1LL << 31) && Mpix % 64 == 0 && N8 >= 64 && (mode != 2 || ws > 0);
    if (mode != 2 && (e.act || e.aux_out || e.gate || e.rowadd || e.out_f32 || e.beta != 0.f || (e.resid && !e.resid_act))) p8 = false;
    if (p8) {
        const P8Plan pl = vaw_p8_plan(M8, N8, K, mode == 2, false, ws, force, cus);
        if (pl.use && (mode != 2 || pl.split >= 2)) {
            p.variant = VAW_GV_PERSISTENT;
            p.ntw = pl.ntw;
            p.epi_kind = mode == 2 ? P8_SLAB : (mode == 0 && e.resid) ? P8_RESID : P8_STORE;
            p.transposed = mode == 2;
            p.M = M8, p.N = N8, p.K = K;
            p.split = pl.split;
            p.grid_x = pl.grid;
            p.block = 512;
            p.lds_bytes = vaw_lds_p8(pl.ntw);
            if (mode == 2) {
                p.reduce = VAW_CVR_SLAB_T;
                p.launches += 1;
                p.workspace_floats_used = (int64_t)pl.split * M8 * N8;
                // bias gradient on the same launch: 192-column kernel only (the 256-column one has no registers left for it)
                if (bias_grad && pl.ntw == 3 && ws >= p.workspace_floats_used + (int64_t)pl.split * N8) {
                    p.bias_grad = VAW_CVB_FUSED;
                    p.workspace_floats_used += (int64_t)pl.split * N8;
                } else if (bias_grad) {      // column sums of dy [pixels][Co], as a pass of its own
                    p.bias_grad = VAW_CVB_SEPARATE;
                    vaw_row_launch rp;
                    const int rc = vaw_row_plan(VAW_ROW_COLSUM, dt, Mpix, 1, Co, Co, act, ws, &rp);
                    if (rc) return rc;
                    if (rp.workspace_floats > p.workspace_floats_used) p.workspace_floats_used = rp.workspace_floats;
                    p.launches += 2;
                }
            }
            *plan = p;
            plan->status = p.status = VAW_OK;
            return VAW_OK;
        }
    }
    // ---- 128 x 128
    const int64_t n_wg = ((M + 127) / 128) * ((N + 127) / 128);
    const bool plain_f32 = mode == 2 && !e.bias && !e.act;
    p.variant = VAW_GV_T128_BK64;
    p.M = M, p.N = N, p.K = K;
    p.split = no_empty_split((int)(K / 64), colsum ? 1 : pick_split(n_wg, K, M * N, ws - (bias_grad ? 64 * M : 0), plain_f32));
    const int64_t slabs = p.split > 1 ? (int64_t)p.split * M * N : 0;
    VAW_CHECK_ARG(!bias_grad || (ws > 0 && ws >= slabs + p.split * M), "conv3x3: bias gradient needs a workspace");
    p.xcd_parts = xcd_parts_for(k, p.split);
    p.grid_x = p.xcd_parts ? (int)(8 * ((n_wg + p.xcd_parts - 1) / p.xcd_parts)) : (int)n_wg;
    p.grid_y = p.xcd_parts ? 1 : p.split;
    p.block = 256;
    p.lds_bytes = vaw_lds_t128(64);
    p.reduce = p.split == 1 ? VAW_CVR_NONE : bias_grad ? VAW_CVR_F32_ROWSUM : VAW_CVR_F32;
    p.bias_grad = !bias_grad ? VAW_CVB_NONE : p.split > 1 ? VAW_CVB_FUSED : VAW_CVB_FOLD;
    p.colsum_mode = colsum ? VAW_GC_FOLD : VAW_GC_NONE;
    p.colsum_rows = colsum ? (M + 127) / 128 : 0;
    p.workspace_floats_used = slabs + (bias_grad ? (int64_t)p.split * M : 0) + p.colsum_rows * N;
    p.launches += (p.reduce != VAW_CVR_NONE) + (p.bias_grad == VAW_CVB_FOLD) + colsum;
    *plan = p;
    plan->status = p.status = VAW_OK;
    return VAW_OK;
}

// Parked-drain persistent GEMM (gemm_pd_kernel.h): dispatch and the forward-layout instantiations
// (A [M][K] activations, B [N][K] weights).  The input-gradient layout lives in gemm_pd_dgrad.hip.
#include "gemm_pd_kernel.h"
#include "gemm_plan.h"
static_assert(PdCfg<3>::lds_bytes == vaw_lds_pd(3) && PdCfg<4>::lds_bytes == vaw_lds_pd(4), "gemm_plan.h: LDS size of the parked-drain kernel");

void pd_launch_dgrad(int ntw, int epi, const bf16_t* a, int64_t lda, const bf16_t* b, int64_t ldb, int nk, int tiles_m, int tiles_n,
                     int grid, const EpiDev& e, hipStream_t s);

// ntw, epi (P8_* kind) and grid come from vaw_gemm_plan (gemm_plan.hip)
void vaw_pd_launch(int ntw, int epi, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda, const bf16_t* b,
                   int64_t ldb, const EpiDev& e, int grid, hipStream_t s) {
    const int bn = 64 * ntw;
    const int tiles_m = (int)((M + PD_BM - 1) / PD_BM), tiles_n = (int)((N + bn - 1) / bn), nk = (int)(K / 64);
    if (!b_kmajor) { pd_launch_dgrad(ntw, epi, a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s); return; }
#define PD_CASE(EPIv)                                                                                   \
    case EPIv:                                                                                          \
        if (ntw == 4) pd_launch_one<true, 4, EPIv>(a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s);   \
        else pd_launch_one<true, 3, EPIv>(a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s);            \
        break
    switch (epi) {
        PD_CASE(P8_STORE);
        PD_CASE(P8_GELU);
        PD_CASE(P8_GATE);
        default: break;
    }
}

// Warp-specialised persistent GEMM (gemm_ws_kernel.h): dispatch and the forward-layout instantiations; the input-gradient layout
// lives in gemm_ws_dgrad.hip.
#include "gemm_ws_kernel.h"
#include "gemm_plan.h"
static_assert(WsCfg<3>::lds_bytes == vaw_lds_ws(3) && WsCfg<4>::lds_bytes == vaw_lds_ws(4), "gemm_plan.h: LDS size of the warp-specialised kernel");

void ws_launch_dgrad(int ntw, int epi, const bf16_t* a, int64_t lda, const bf16_t* b, int64_t ldb, int nk, int tiles_m, int tiles_n,
                     int grid, bool loaders8, const EpiDev& e, hipStream_t s);

// ntw, epi (P8_* kind), grid and loaders8 (VAW_WS_LOADERS=8: the 192-column kernels with eight loader waves, 16 waves per
// workgroup, instead of four) come from vaw_gemm_plan
void vaw_ws_launch(int ntw, int epi, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda, const bf16_t* b,
                   int64_t ldb, const EpiDev& e, int grid, bool loaders8, hipStream_t s) {
    const int bn = 64 * ntw;
    const int tiles_m = (int)((M + WS_BM - 1) / WS_BM), tiles_n = (int)((N + bn - 1) / bn), nk = (int)(K / 64);
    if (!b_kmajor) { ws_launch_dgrad(ntw, epi, a, lda, b, ldb, nk, tiles_m, tiles_n, grid, loaders8, e, s); return; }
#define WS_CASE(EPIv)                                                                                   \
    case EPIv:                                                                                          \
        if (ntw == 4) ws_launch_one<true, 4, EPIv>(a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s);   \
        else if (loaders8) ws_launch_one<true, 3, EPIv, 8>(a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s);   \
        else ws_launch_one<true, 3, EPIv>(a, lda, b, ldb, nk, tiles_m, tiles_n, grid, e, s);            \
        break
    switch (epi) {
        WS_CASE(P8_STORE);
        WS_CASE(P8_GELU);
        WS_CASE(P8_GATE);
        default: break;
    }
}

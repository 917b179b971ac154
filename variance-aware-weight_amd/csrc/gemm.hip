// Dense contraction kernels (the >97 % of DiT FLOPs):  C[M,N] = epilogue(alpha * op(A) . op(B)).
//
//   gemm_bf16_kernel   bf16 operands, v_mfma_f32_16x16x32_bf16, 128x128x64 block tile, 4 waves (2x2) of
//                      64x64, both operand tiles brought in by LDS-DMA (global_load_lds_dwordx4) into a
//                      double-buffered, XOR-swizzled LDS image (swizzle on the per-lane SOURCE address;
//                      the LDS side of an LDS-DMA is lane-linear), one barrier per K step.
//                      k-major operands ([rows][K]) are read with ds_read_b128, mn-major operands
//                      ([K][rows]: dgrad's W, wgrad's dY and X) with the ds_read_b64_tr_b16 hardware
//                      transpose, so forward, dgrad and wgrad run the same loop with no transposed copies.
//   gemm_generic_kernel any shape / alignment / dtype: register-staged, f32 LDS image, exact-f32
//                      v_mfma_f32_16x16x4_f32.  Serves the f32 parity mode and the odd shapes
//                      (N = p*p*C = 64 head, tiny test models).
//
// MFMA operand maps used (cdna_hip_programming.md §3):
//   16x16x32 bf16: lane l holds A[row l&15][k = 8(l>>4)+j], B[k = 8(l>>4)+j][col l&15], j=0..7
//   16x16x4  f32 : lane l holds A[row l&15][k = l>>4],       B[k = l>>4][col l&15]
//   C/D (both)   : col = l&15, row = 4(l>>4) + reg
#include "common.h"
#include <type_traits>

#include "gemm_plan.h"

// =============================================================================================
// Fast path: bf16, M%128==0, N%128==0, K%64==0, 16-byte aligned rows.
// Template BKT = K depth of one pipeline stage:
//   64: 2 x 32 KiB of operand tiles, 2 workgroups per CU -- long-K launches (weight gradients)
//   32: 2 x 16 KiB, epilogue staged in two 64-row halves (33 KiB) -> up to 4 workgroups per CU, so that the
//       HBM-bound epilogue of one workgroup overlaps the MFMA loop of the others -- short-K launches (K = 768)
// =============================================================================================
#define BM 128
#define BN 128
#define BK 64                       // granularity the dispatcher requires of K
#define CS_LD 132                   // f32 row stride of the epilogue staging image (128 + 4: conflict-free)
#define CS_BYTES (64 * CS_LD * 4)   // one 64-row half: 33,792 B
#define CP_BYTES (4 * 128 * 4)      // column-sum scratch

template <int BKT> struct FastCfg {
    static constexpr int tile_bytes = 128 * BKT * 2;
    static constexpr int stage_bytes = 2 * tile_bytes;
    static constexpr int main_bytes = 2 * stage_bytes;
    static constexpr int lds_bytes = (main_bytes > CS_BYTES ? main_bytes : CS_BYTES) + CP_BYTES;
};

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// k-major image [128 rows][BKT/8 chunks of 16 B].  The XOR keeps every 16-lane group of a ds_read_b128 of the
// 16x16x32 fragment (row = l&15, chunk = 4s + (l>>4)) on 16 distinct 16-byte slots of the 256-byte bank row:
//   BKT=64 (128-B rows): chunk' = chunk ^ ((row>>1)&7);   BKT=32 (64-B rows): chunk' = chunk ^ ((-(row>>2))&3)
template <int BKT>
__device__ __forceinline__ int kmaj_swz(int row) { return BKT == 64 ? ((row >> 1) & 7) : ((-(row >> 2)) & 3); }
template <int BKT>
__device__ __forceinline__ int kmaj_off(int row, int chunk) { return row * (2 * BKT) + ((chunk ^ kmaj_swz<BKT>(row)) << 4); }
// mn-major image: [BKT k-rows][16 chunks of 16 B]; chunk' = chunk ^ (((row&3)<<2)|((row>>2)&3))
//   (image (b) of cdna_hip_programming.md T10: conflict-free ds_read_b64_tr_b16 for the 16x16x32 operand)
__device__ __forceinline__ int mnmaj_off(int row, int chunk) {
    return row * 256 + ((chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

// Stage one 128 x BKT (k-major) or BKT x 128 (mn-major) operand tile into LDS by LDS-DMA: BKT/4 wave-instructions
// of 1 KiB, BKT/16 per wave.  g points at the tile's first element; ld = leading dimension in elements.
template <bool KMAJOR, int BKT>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ g, int64_t ld, char* lds_tile, int wid, int lane,
                                           int valid) {
    // `valid` = rows (k-major) or columns (mn-major, multiple of 8) of this 128-wide tile that exist in the matrix.
    // Out-of-range lanes re-read an in-range chunk instead (LDS-DMA cannot zero-fill): the duplicate data only
    // reaches accumulator rows/columns that the epilogue never stores.
    constexpr int PER_WAVE = BKT / 16;
    constexpr int CPR = BKT / 8;             // 16-byte chunks per k-major row
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const int inst = wid * PER_WAVE + i;
        const bf16_t* src;
        if (KMAJOR) {
            int row = inst * (64 / CPR) + lane / CPR;
            const int chunk = (lane % CPR) ^ kmaj_swz<BKT>(row);
            row = row < valid ? row : valid - 1;
            src = g + (int64_t)row * ld + chunk * 8;
        } else {
            const int row = inst * 4 + (lane >> 4);
            int chunk = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
            chunk = chunk * 8 < valid ? chunk : 0;
            src = g + (int64_t)row * ld + chunk * 8;
        }
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(lds_tile + inst * 1024), 16, 0, 0);
    }
}

// Fragment of 16 (rows) x 32 (k) for k-substep s of the tile rows r0..r0+15.
template <bool KMAJOR, int BKT>
__device__ __forceinline__ bf16x8 load_frag(const char* lds_tile, int r0, int s, int lane) {
    if (KMAJOR) {
        const int row = r0 + (lane & 15);
        return *reinterpret_cast<const bf16x8*>(lds_tile + kmaj_off<BKT>(row, 4 * s + (lane >> 4)));
    } else {
        const int li = lane & 15, q = li >> 2, p = li & 3;
        const int kb = 32 * s + 8 * (lane >> 4) + q;
        const int ch = (r0 >> 3) + (p >> 1);
        const char* a0 = lds_tile + mnmaj_off(kb, ch) + 8 * (p & 1);
        const char* a1 = lds_tile + mnmaj_off(kb + 4, ch) + 8 * (p & 1);
        bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)a0);
        bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)a1);
        bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return r;
    }
}

// ---- implicit-GEMM conv3x3 (stride 1, pad 1) on NHWC activations: the patch matrix is never materialised; the LDS-DMA
// source address of each 16-byte chunk is computed from (pixel, tap, channel) and padding taps read a zero page.
//   CONV 1 (forward)        A[m][k=(tap,ci)]  = x[pix(m)+s(tap)][ci]                      B = W[co][(tap,ci)] (plain, k-major)
//   CONV 2 (input gradient) A[m][k=(tap,co)]  = dy[pix(m)+s(tap)][co]                     B[k][n=ci] = W[co][8-tap][ci]  (mn-major slice)
//   CONV 3 (weight gradient) A = dy^T (plain, mn-major)                                   B[k=m][n=(tap,ci)] = x[pix(m)+s(tap)][ci] (mn-major)
// K tiles never straddle a tap: Ci (CONV 1) / Co (CONV 2) is a multiple of the stage depth.
struct ConvGeom {
    int H, W, Ci, Co;
};
__device__ __attribute__((aligned(64))) const unsigned char vaw_zero_page[64] = {0};

#define KMAJ_READS(KM) ((KM) ? 1 : 2)      /* LDS read instructions per fragment: one b128, or two transposing b64 */
template <bool AK, bool BKM, int BKT, int CONV>
__global__ void __launch_bounds__(256, BKT == 64 ? 2 : 3)
gemm_bf16_kernel(const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb, int nk_total,
                 int tiles_n, int n_wg, int n_split, EpiDev e, ConvGeom cg, int xcd_parts) {
    using Cfg = FastCfg<BKT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][A tile | B tile]; reused by the epilogue
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware remap: workgroups b, b+8, ... share an XCD (round-robin dispatch) and its 4 MiB L2.
    //   xcd_parts == 0: 2-D grid (tiles, splits); each XCD gets a contiguous run of tiles (bijective for any grid) so
    //     A row-panels are re-read from that XCD's L2.
    //   xcd_parts == 8 / n_split (n_split in {2, 4, 8}; 1-D grid of 8 * ceil(n_wg / xcd_parts) workgroups): XCD x works on
    //     ONE K range (x % n_split) of ONE contiguous part of the tiles (x / n_split), so the workgroups sharing an L2
    //     walk the same K range in step and every operand panel of that range is fetched once for all of them
    //     (split-K weight gradients: measured HBM fetch was 3x the operand bytes with the tile-run mapping).
    int wg, split_idx;
    if (xcd_parts > 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, per = (n_wg + xcd_parts - 1) / xcd_parts;
        split_idx = xcd % n_split;
        wg = (xcd / n_split) * per + j;
        if (j >= per || wg >= n_wg) return;      // padding workgroups of the last part (uniform: before any barrier)
    } else {
        const int orig = blockIdx.x, xcd = orig & 7, q = n_wg >> 3, r = n_wg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        split_idx = blockIdx.y;
    }
    // Within an XCD's run, walk the tiles in groups of 8 row panels (row fastest): the workgroups resident on
    // an XCD then touch ~8 A panels + ~8 B panels (3 MB at K=768), which stay in its 4 MiB L2.
    int tm, tn;
    {
        const int tiles_m = n_wg / tiles_n, per_group = 8 * tiles_n;   // n_wg = tiles_m * tiles_n exactly
        const int group = wg / per_group, first_m = group * 8;
        const int gsize = tiles_m - first_m < 8 ? tiles_m - first_m : 8;
        const int in_group = wg - group * per_group;
        tm = first_m + in_group % gsize;
        tn = in_group / gsize;
    }
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    const int64_t a_step = AK ? BKT : (int64_t)BKT * lda;       // step along k: +BKT (k-major) or +BKT*lda
    const int64_t b_step = BKM ? BKT : (int64_t)BKT * ldb;
    // split-K: split_idx owns k-tiles [kt0, kt0 + nk)   (nk_total counts BKT-deep tiles)
    const int nk_per = (nk_total + n_split - 1) / n_split;
    const int kt0 = split_idx * nk_per;
    const int nk = e.debug == 2 ? 1 : (kt0 + nk_per <= nk_total ? nk_per : nk_total - kt0);
    const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
    const int mvalid = e.M - m0 < BM ? (int)(e.M - m0) : BM;     // edge tiles: rows / columns that exist
    const int nvalid = e.N - n0 < BN ? (int)(e.N - n0) : BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

    // ---- per-lane constants of the gather modes (pixel coordinates of the rows / columns this lane stages) ----
    constexpr int PW = BKT / 16, CPR = BKT / 8;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(vaw_zero_page);
    int ga_h[PW], ga_w[PW];
    int64_t ga_pix[PW];
    if (CONV == 1 || CONV == 2) {
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            int row = (wid * PW + i) * (64 / CPR) + lane / CPR;
            row = row < mvalid ? row : mvalid - 1;
            const int64_t p = m0 + row;
            ga_pix[i] = p * (CONV == 1 ? cg.Ci : cg.Co) + (((lane % CPR) ^ kmaj_swz<BKT>((wid * PW + i) * (64 / CPR) + lane / CPR)) << 3);
            ga_w[i] = (int)(p % cg.W);
            ga_h[i] = (int)((p / cg.W) % cg.H);
        }
    }
    // CONV 3: the pixel (h, w) and source offset of the row each lane stages are carried from K tile to K tile
    // (64 pixels further on each time) instead of being divided out of the pixel index at every step.
    int gb_dh[PW], gb_dw[PW], gb_h[PW], gb_w[PW];
    int64_t gb_off[PW];
    const int step_w = CONV == 3 ? BKT % cg.W : 0, step_h = CONV == 3 ? (BKT / cg.W) % cg.H : 0;
    if (CONV == 3) {
        const int nk_per0 = (nk_total + n_split - 1) / n_split;
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int row = (wid * PW + i) * 4 + (lane >> 4);
            const int chunk = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
            const int n = (int)n0 + chunk * 8;
            const int tap = n < e.N ? n / cg.Ci : -1;     // -1: column beyond 9*Ci (edge tile) -> zero page
            gb_dh[i] = tap >= 0 ? tap / 3 - 1 : (1 << 20);
            gb_dw[i] = tap >= 0 ? tap % 3 - 1 : 0;
            const int64_t p = (int64_t)split_idx * nk_per0 * BKT + row;
            gb_w[i] = (int)(p % cg.W);
            gb_h[i] = (int)((p / cg.W) % cg.H);
            gb_off[i] = tap >= 0 ? (p + (int64_t)gb_dh[i] * cg.W + gb_dw[i]) * cg.Ci + n % cg.Ci : 0;
        }
    }
    // CONV 1/2: (tap, first channel) of the K tile about to be staged, carried from tile to tile (A and B side alike)
    const int conv_cin = CONV == 1 ? cg.Ci : cg.Co;
    int a_tap = 0, a_c0 = 0, b_tap = 0, b_c0 = 0;
    if (CONV == 1 || CONV == 2) {
        const int kglob = split_idx * ((nk_total + n_split - 1) / n_split) * BKT;
        a_tap = b_tap = kglob / conv_cin;
        a_c0 = b_c0 = kglob - a_tap * conv_cin;
    }
    auto stage_a = [&](int ktile, char* dst) {        // ktile counts BKT-deep tiles from k = 0; consecutive calls only
        if (CONV == 1 || CONV == 2) {
            const int cin = conv_cin;
            const int tap = a_tap, c0 = a_c0;
            a_c0 += BKT;
            if (a_c0 >= cin) { a_c0 = 0; a_tap += 1; }
            const int dh = tap / 3 - 1, dw = tap % 3 - 1;
            const bf16_t* a_tap_base = A + ((int64_t)dh * cg.W + dw) * cin + c0;     // uniform: one scalar add per piece
#pragma unroll
            for (int i = 0; i < PW; ++i) {
                const int inst = wid * PW + i;
                const int hh = ga_h[i] + dh, ww = ga_w[i] + dw;
                const bool in = hh >= 0 && hh < cg.H && ww >= 0 && ww < cg.W;
                const bf16_t* src = in ? a_tap_base + ga_pix[i] : zero;   // ga_pix: element offset of (pixel, swizzled chunk)
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(dst + inst * 1024), 16, 0, 0);
            }
        } else {
            stage_tile<AK, BKT>((AK ? A + m0 * lda : A + m0) + ktile * a_step, lda, dst, wid, lane, mvalid);
        }
    };
    auto stage_b = [&](int ktile, char* dst) {
        if (CONV == 2) {                              // W[co][8-tap][ci]: rows = co, row stride 9*Ci, tap picks the column window
            const int tap = b_tap, c0 = b_c0;
            b_c0 += BKT;
            if (b_c0 >= cg.Co) { b_c0 = 0; b_tap += 1; }
            stage_tile<false, BKT>(B + (int64_t)c0 * ldb + (8 - tap) * cg.Ci + n0, ldb, dst, wid, lane, nvalid);
        } else if (CONV == 3) {       // called for consecutive K tiles only: the per-lane state advances by one tile
#pragma unroll
            for (int i = 0; i < PW; ++i) {
                const int inst = wid * PW + i;
                const int hh = gb_h[i] + gb_dh[i], ww = gb_w[i] + gb_dw[i];
                const bool in = hh >= 0 && hh < cg.H && ww >= 0 && ww < cg.W;
                const bf16_t* src = in ? B + gb_off[i] : zero;
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(dst + inst * 1024), 16, 0, 0);
                gb_off[i] += (int64_t)BKT * cg.Ci;
                gb_w[i] += step_w;
                if (gb_w[i] >= cg.W) { gb_w[i] -= cg.W; gb_h[i] += 1; }
                gb_h[i] += step_h;
                if (gb_h[i] >= cg.H) gb_h[i] -= cg.H;
            }
        } else {
            stage_tile<BKM, BKT>((BKM ? B + n0 * ldb : B + n0) + ktile * b_step, ldb, dst, wid, lane, nvalid);
        }
    };
    const bool wave_live = wm < mvalid && wn < nvalid;
    constexpr bool CAN_ROWSUM = CONV == 3 || (CONV == 0 && !AK);
    const bool do_rowsum = CAN_ROWSUM && e.rowpart != nullptr && tn == 0 && wn == 0;   // one column of tiles, its two left waves
    f32x4 accr[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    const bf16x8 ones8 = {(bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f, (bf16_t)1.f};
    stage_a(kt0, smem);
    stage_b(kt0, smem + Cfg::tile_bytes);
    // The K loop exists twice (compile-time flag): the few waves that also take row sums of A (CONV 3 bias gradient) run
    // their own copy, so the common copy's schedule and register use are untouched by it.
    auto k_loop = [&](auto with_rowsum, auto with_preload) {
        constexpr bool RS = decltype(with_rowsum)::value, PRE = decltype(with_preload)::value;
        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA for tile kt has landed
            __syncthreads();                                    // everyone's has; and tile kt-1 is no longer read
            char* cur = smem + (kt & 1) * Cfg::stage_bytes;
            if (kt + 1 < nk) {
                char* nxt = smem + ((kt + 1) & 1) * Cfg::stage_bytes;
                stage_a(kt0 + kt + 1, nxt);
                stage_b(kt0 + kt + 1, nxt + Cfg::tile_bytes);
            }
            if (!wave_live) continue;      // this wave's 64 x 64 quadrant lies wholly outside the matrix (edge tile)
            if (PRE) {
                // every fragment of the K tile is requested before the first MFMA: the LDS latency of the second 32-deep
                // half hides behind the MFMAs of the first instead of being waited for in the open
                bf16x8 afp[BKT / 32][4], bfp[BKT / 32][4];
#pragma unroll
                for (int s = 0; s < BKT / 32; ++s) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) bfp[s][j] = load_frag<BKM, BKT>(cur + Cfg::tile_bytes, wn + 16 * j, s, lane);
#pragma unroll
                    for (int i = 0; i < 4; ++i) afp[s][i] = load_frag<AK, BKT>(cur, wm + 16 * i, s, lane);
                }
#pragma unroll
                for (int s = 0; s < BKT / 32; ++s)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfp[s][j], afp[s][i], acc[i][j], 0, 0, 0);
                // pin the order: all LDS reads of the tile first, then the MFMAs (mask 0x100 = DS read, 0x008 = MFMA)
                __builtin_amdgcn_sched_group_barrier(0x100, (KMAJ_READS(AK) + KMAJ_READS(BKM)) * 4 * (BKT / 32), 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 16 * (BKT / 32), 0);
                continue;
            }
#pragma unroll
            for (int s = 0; s < BKT / 32; ++s) {
                bf16x8 af[4], bfr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = load_frag<AK, BKT>(cur, wm + 16 * i, s, lane);
#pragma unroll
                for (int j = 0; j < 4; ++j) bfr[j] = load_frag<BKM, BKT>(cur + Cfg::tile_bytes, wn + 16 * j, s, lane);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        // operands swapped: the tile is accumulated TRANSPOSED (lane l: row m = l&15, columns 4(l>>4)..+3),
                        // so the epilogue finds 4 consecutive output columns in one register quad
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                if (RS) {     // ones . A^T: every row of the 16 x 16 result holds the row sums of A
#pragma unroll
                    for (int i = 0; i < 4; ++i) accr[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, af[i], accr[i], 0, 0, 0);
                }
            }
        }
    };
    if (CAN_ROWSUM && do_rowsum) k_loop(std::true_type{}, std::false_type{});
    else if (BKT == 32 && CONV == 0 && AK) k_loop(std::false_type{}, std::true_type{});   // measured: +3..8 % on the 32-deep
                                                                                            // input-gradient launches, neutral elsewhere
    else k_loop(std::false_type{}, std::false_type{});
    if (CAN_ROWSUM && do_rowsum && lane < 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm + 16 * i + lane;
            if (row < mvalid) e.rowpart[(int64_t)split_idx * e.M + m0 + row] = accr[i][0];
        }
    }
    if (e.debug == 1) {   // keep the accumulators alive with one store per wave-quadrant
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        if (t == 12345.678f) ((float*)e.C)[0] = t;
        return;
    }
    // ---- direct epilogue: every lane owns rows (l&15) of its 4 m-tiles and 4 consecutive columns per n-tile ----
    // (measured: a win only for the f32 split-K partials -- 16 B per lane, 64-B row segments; bf16 outputs written 8 B
    //  per lane in 32-B segments ran 1.5-2x slower than the LDS-staged 16-B rows below, so those keep the staging)
    if (e.direct_epi && !e.colpart && n_split > 1) {
        if (!wave_live) return;
        const int g4 = 4 * (lane >> 4), lr = lane & 15;
        float* slab = n_split > 1 ? e.slab + (int64_t)split_idx * e.M * e.N : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wn + 16 * j + g4;
            if (col >= nvalid) continue;
            const f32x4 bj = (e.bias && n_split == 1) ? load4(e.bias + n0 + col) : f32x4{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm + 16 * i + lr;
                if (row >= mvalid) continue;
                if (n_split > 1) store4(slab + (m0 + row) * e.N + n0 + col, acc[i][j]);
                else epi_row4(e, (unsigned)(m0 + row), n0 + col, acc[i][j], bj);
            }
        }
        return;
    }
    // ---- epilogue in two 64-row halves: accumulators -> f32 staging image in LDS (the operand tiles are dead),
    //      then each thread owns 8 consecutive columns of one row per pass: 16-byte loads and stores ----
    float* cs = reinterpret_cast<float*>(smem);
    const int c8 = (threadIdx.x & 15) * 8, r0 = threadIdx.x >> 4;
    const bool col_ok = c8 < nvalid;             // N % 8 == 0: an 8-column group is in or out as a whole
    f32x4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
    if (e.bias && n_split == 1 && col_ok) {
        b0 = load4(e.bias + n0 + c8);
        b1 = load4(e.bias + n0 + c8 + 4);
    }
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        if ((wid >> 1) == half) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    store4(cs + (16 * i + (lane & 15)) * CS_LD + wn + 16 * j + 4 * (lane >> 4), acc[i][j]);
        }
        __syncthreads();
        if (n_split > 1) {
            float* slab = e.slab + (int64_t)split_idx * e.M * e.N;
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int row = pass * 16 + r0;
                if (!col_ok || 64 * half + row >= mvalid) continue;
                const float* src = cs + row * CS_LD + c8;
                float* dst = slab + (m0 + 64 * half + row) * e.N + n0 + c8;
                store4(dst, load4(src));        // split-K partials are re-read at once by the reduce: keep them cached
                store4(dst + 4, load4(src + 4));
            }
        } else {
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int row = pass * 16 + r0;
                if (!col_ok || 64 * half + row >= mvalid) continue;
                const float* src = cs + row * CS_LD + c8;
                f32x4 v0 = load4(src), v1 = load4(src + 4);
                epi_row8(e, (unsigned)(m0 + 64 * half + row), n0 + c8, v0, v1, b0, b1);
                s0 += v0;
                s1 += v1;
            }
        }
    }
    if (e.colpart && n_split == 1) {
        // fold the 16 row-threads of each 8-column group in a fixed order: 4 in-wave (xor 16, 32), then 4 waves via LDS
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s0[j] += __shfl_xor(s0[j], 16, 64); s0[j] += __shfl_xor(s0[j], 32, 64);
            s1[j] += __shfl_xor(s1[j], 16, 64); s1[j] += __shfl_xor(s1[j], 32, 64);
        }
        float* cp = reinterpret_cast<float*>(smem + Cfg::lds_bytes - CP_BYTES);   // [4 waves][128]
        if (lane < 16) {
            store4(cp + wid * 128 + c8, s0);
            store4(cp + wid * 128 + c8 + 4, s1);
        }
        __syncthreads();
        if (threadIdx.x < nvalid)
            e.colpart[(int64_t)tm * e.N + n0 + threadIdx.x] =
                ((cp[threadIdx.x] + cp[128 + threadIdx.x]) + cp[256 + threadIdx.x]) + cp[384 + threadIdx.x];
    }
}

// =============================================================================================
// Large-tile variant: 256 x 256 block tile, 8 waves (2 x 4, each 128 x 64 = 8 x 4 MFMA tiles), ONE workgroup per
// CU, K in 32-deep tiles through a ring of FOUR 32 KiB LDS stages filled by LDS-DMA.
// Why: the ablations in DESIGN.md ("GEMM main loop") show the 128 x 128 kernel is bound by the vector-memory ->
// LDS path (64 B/clk/CU) and by LDS bandwidth, not by MFMA issue: per MFMA cycle it moves 2x the global bytes
// and 1.33x the LDS fragment bytes of this shape.  The loads of K tile t+3 are issued before the MFMAs of tile t and
// only waited for with a COUNTED s_waitcnt vmcnt(8) (4 LDS-DMA instructions per wave per tile, two tiles may stay
// in flight) followed by a raw s_barrier (__syncthreads() would drain vmcnt to 0; cdna_hip_programming.md
// "Pipelining across barriers").
// Each operand tile is two 128-wide images of the kinds above (same swizzles, same fragment loads).
// =============================================================================================
#define BIG_BM 256
#define BIG_BN 256
#define BIG_IMG (128 * 32 * 2)                  // one 128 x 32 image: 8 KiB
#define BIG_STAGE (4 * BIG_IMG)                 // A img0 | A img1 | B img0 | B img1 = 32 KiB
#define BIG_NSTAGE 4
#define BIG_CS_LD 260                           // f32 row stride of the epilogue staging image (256 + 4)
#define BIG_LDS (BIG_NSTAGE * BIG_STAGE + 8 * 256 * 4)   // ring (also the 64 x 260 f32 epilogue image) + column sums

template <bool AK, bool BKM>
__global__ void __launch_bounds__(512, 1)
gemm_bf16_big_kernel(const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb, int nk_total,
                     int tiles_n, int n_wg, int n_split, EpiDev e) {
    constexpr int BKT = 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // 0..7
    int wg;
    {
        const int orig = blockIdx.x, xcd = orig & 7, q = n_wg >> 3, r = n_wg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    int tm, tn;
    {
        const int tiles_m = n_wg / tiles_n, per_group = 4 * tiles_n;      // 4 row panels of 256 per group
        const int group = wg / per_group, first_m = group * 4;
        const int gsize = tiles_m - first_m < 4 ? tiles_m - first_m : 4;
        const int in_group = wg - group * per_group;
        tm = first_m + in_group % gsize;
        tn = in_group / gsize;
    }
    const int64_t m0 = (int64_t)tm * BIG_BM, n0 = (int64_t)tn * BIG_BN;
    const int nk_per = (nk_total + n_split - 1) / n_split;                // nk_total counts 32-deep tiles
    const int kt0 = blockIdx.y * nk_per;
    const int nk = kt0 + nk_per <= nk_total ? nk_per : nk_total - kt0;
    const int mvalid = e.M - m0 < BIG_BM ? (int)(e.M - m0) : BIG_BM;
    const int nvalid = e.N - n0 < BIG_BN ? (int)(e.N - n0) : BIG_BN;
    const int wy = wid >> 2, wx = wid & 3;                                // wave tile: rows 128*wy.., cols 64*wx..

    // ---- staging: wave w fills (2 pieces each) image w>>2 of A and image w>>2 of B as sub-wave w&3 ----
    const int img = wid >> 2, sw = wid & 3;
    int a_valid = mvalid - 128 * img, b_valid = nvalid - 128 * img;
    const int a_img = a_valid > 0 ? img : 0, b_img = b_valid > 0 ? img : 0;   // image wholly outside: mirror image 0
    a_valid = a_valid > 0 ? (a_valid < 128 ? a_valid : 128) : (mvalid < 128 ? mvalid : 128);
    b_valid = b_valid > 0 ? (b_valid < 128 ? b_valid : 128) : (nvalid < 128 ? nvalid : 128);
    const bf16_t* a_base = AK ? A + (m0 + 128 * a_img) * lda : A + m0 + 128 * a_img;
    const bf16_t* b_base = BKM ? B + (n0 + 128 * b_img) * ldb : B + n0 + 128 * b_img;
    const int64_t a_step = AK ? BKT : (int64_t)BKT * lda;
    const int64_t b_step = BKM ? BKT : (int64_t)BKT * ldb;
    auto stage = [&](int ktile, char* dst) {
        stage_tile<AK, BKT>(a_base + ktile * a_step, lda, dst + img * BIG_IMG, sw, lane, a_valid);
        stage_tile<BKM, BKT>(b_base + ktile * b_step, ldb, dst + (2 + img) * BIG_IMG, sw, lane, b_valid);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

    stage(kt0, smem);
    if (nk > 1) stage(kt0 + 1, smem + BIG_STAGE);
    if (nk > 2) stage(kt0 + 2, smem + 2 * BIG_STAGE);
    const int a_off = wy * BIG_IMG, b_off = (2 + (wx >> 1)) * BIG_IMG, b_row0 = (wx & 1) * 64;
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt landed; tiles kt+1, kt+2 may still fly (4 LDS-DMA instructions per wave per tile)
        if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // every wave's pieces of tile kt are in; nobody still reads tile kt-1
        if (kt + 3 < nk) stage(kt0 + kt + 3, smem + ((kt + 3) & 3) * BIG_STAGE);   // slot of tile kt-1
        const char* cur = smem + (kt & 3) * BIG_STAGE;
        bf16x8 af[8], bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = load_frag<BKM, BKT>(cur + b_off, b_row0 + 16 * j, 0, lane);
#pragma unroll
        for (int i = 0; i < 8; ++i) af[i] = load_frag<AK, BKT>(cur + a_off, 16 * i, 0, lane);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (e.debug == 1) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        if (t == 12345.678f) ((float*)e.C)[0] = t;
        return;
    }
    // ---- epilogue: four 64-row quarters through the (now idle) ring; a thread owns 8 consecutive columns ----
    float* cs = reinterpret_cast<float*>(smem);
    const int c8 = (threadIdx.x & 31) * 8, r0 = threadIdx.x >> 5;       // 16 row-threads x 32 column groups
    const bool col_ok = c8 < nvalid;
    f32x4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
    if (e.bias && n_split == 1 && col_ok) {
        b0 = load4(e.bias + n0 + c8);
        b1 = load4(e.bias + n0 + c8 + 4);
    }
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
#pragma unroll
    for (int quarter = 0; quarter < 4; ++quarter) {
        __syncthreads();
        if (wy == (quarter >> 1)) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        cs[(16 * i + 4 * (lane >> 4) + r) * BIG_CS_LD + 64 * wx + 16 * j + (lane & 15)] =
                            acc[4 * (quarter & 1) + i][j][r];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int row = pass * 16 + r0;
            if (!col_ok || 64 * quarter + row >= mvalid) continue;
            const float* src = cs + row * BIG_CS_LD + c8;
            const int64_t m = m0 + 64 * quarter + row;
            if (n_split > 1) {
                float* dst = e.slab + (int64_t)blockIdx.y * e.M * e.N + m * e.N + n0 + c8;
                store4(dst, load4(src));        // split-K partials are re-read at once by the reduce: keep them cached
                store4(dst + 4, load4(src + 4));
            } else {
                f32x4 v0 = load4(src), v1 = load4(src + 4);
                epi_row8(e, (unsigned)m, n0 + c8, v0, v1, b0, b1);
                s0 += v0;
                s1 += v1;
            }
        }
    }
    if (e.colpart && n_split == 1) {
        // 16 row-threads per column group: 2 in-wave (lane bit 5), then the 8 waves through LDS, fixed order
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s0[j] += __shfl_xor(s0[j], 32, 64);
            s1[j] += __shfl_xor(s1[j], 32, 64);
        }
        float* cp = reinterpret_cast<float*>(smem + BIG_NSTAGE * BIG_STAGE);   // [8 waves][256]
        if (lane < 32) {
            store4(cp + wid * 256 + c8, s0);
            store4(cp + wid * 256 + c8 + 4, s1);
        }
        __syncthreads();
        if ((int)threadIdx.x < nvalid && threadIdx.x < 256) {
            float t = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) t += cp[w8 * 256 + threadIdx.x];
            e.colpart[(int64_t)tm * e.N + n0 + threadIdx.x] = t;
        }
    }
}

// out = beta*C + alpha * sum_s slab[s], fixed order (deterministic split-K).  N % 4 == 0.
// The grid also folds the [S][M] partial row sums of A (bias gradient), when given: one launch fewer.
template <typename TO>
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, int S, int64_t M, int64_t N, int64_t ldc,
                                     void* __restrict__ C, float alpha, float beta, int out_f32,
                                     const float* __restrict__ rowpart = nullptr, float* __restrict__ rowsum_out = nullptr,
                                     float rowsum_beta = 0.f) {
    if (rowpart) {
        // one row sum per thread of the whole grid, eight slabs requested at once and added in slab order (round 4 left all M rows
        // to the last workgroup, one dependent load at a time: 51 us for the patch embedding's 768 rows x 64 slabs)
        for (int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
            float t = 0.f;
            int sidx = 0;
            for (; sidx + 8 <= S; sidx += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = rowpart[(int64_t)(sidx + u) * M + m];
#pragma unroll
                for (int u = 0; u < 8; ++u) t += v[u];
            }
            for (; sidx < S; ++sidx) t += rowpart[(int64_t)sidx * M + m];
            rowsum_out[m] = (rowsum_beta != 0.f ? rowsum_beta * rowsum_out[m] : 0.f) + t;
        }
    }
    const int64_t total4 = M * N / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = (4 * i) / N, n = (4 * i) % N;
        f32x4 acc = {0, 0, 0, 0};
        // eight slabs requested at once, added in slab order (the sum is the sequential one; only the loads overlap: the small
        // outputs of the long-K launches -- adaLN input gradient, patch-embed / final-layer weight gradients -- give this kernel a
        // few hundred threads each walking 64 slabs, 38 us per call in round 3 with one load in flight)
        int sidx = 0;
        for (; sidx + 8 <= S; sidx += 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = load4(slab + (int64_t)(sidx + u) * M * N + 4 * i);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; sidx < S; ++sidx) acc += load4(slab + (int64_t)sidx * M * N + 4 * i);
        acc *= alpha;
        const int64_t off = m * ldc + n;
        if (out_f32) {
            float* c = (float*)C + off;
            if (beta != 0.f) acc += beta * load4(c);
            store4(c, acc);
        } else {
            store4((TO*)C + off, acc);
        }
    }
}

// =============================================================================================
// Generic path: any shape; operands f32 or bf16 converted to an f32 LDS image [k][m], stride 144.
// =============================================================================================
#define GBM 128
#define GBN 128
#define GBK 16
#define GLD 144   // 128 + 16: lanes l and l+16 (next k) land on disjoint bank halves for ds_read_b32

template <typename T, bool KMAJOR>
__device__ __forceinline__ void generic_stage(const T* __restrict__ g, int64_t ld, int64_t r0, int64_t rows, int64_t k0,
                                              int64_t K, float* tile, int tid) {
#pragma unroll
    for (int i = 0; i < (GBM * GBK) / 256; ++i) {
        const int e = tid + 256 * i;
        int r, k;
        if (KMAJOR) { r = e / GBK; k = e % GBK; } else { k = e / GBM; r = e % GBM; }
        const int64_t gr = r0 + r, gk = k0 + k;
        float v = 0.f;
        if (gr < rows && gk < K) v = to_f32(KMAJOR ? g[gr * ld + gk] : g[gk * ld + gr]);
        tile[k * GLD + r] = v;
    }
}

template <typename T, bool AK, bool BKM>
__global__ void __launch_bounds__(256)
gemm_generic_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, int64_t K, int64_t kchunk,
                    EpiDev e) {
    __shared__ float As[GBK * GLD];
    __shared__ float Bs[GBK * GLD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.y * GBM, n0 = (int64_t)blockIdx.x * GBN;
    const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    const int64_t kbeg = (int64_t)blockIdx.z * kchunk;
    const int64_t kend = kbeg + kchunk < K ? kbeg + kchunk : K;
    for (int64_t k0 = kbeg; k0 < kend; k0 += GBK) {
        __syncthreads();
        generic_stage<T, AK>(A, lda, m0, e.M, k0, kend, As, tid);
        generic_stage<T, BKM>(B, ldb, n0, e.N, k0, kend, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GBK / 4; ++s) {
            const int kk = 4 * s + (lane >> 4);
            float af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[kk * GLD + wm + 16 * i + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = Bs[kk * GLD + wn + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    if (gridDim.z > 1) {   // split-K: raw partial sums to this split's slab
        float* slab = e.slab + (int64_t)blockIdx.z * e.M * e.N;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t n = n0 + wn + 16 * j + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = m0 + wm + 16 * i + 4 * (lane >> 4) + r;
                    if (m < e.M && n < e.N) slab[m * e.N + n] = acc[i][j][r];
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            epi_store4<T>(e, m0 + wm + 16 * i + 4 * (lane >> 4), n0 + wn + 16 * j + (lane & 15), acc[i][j]);
}

// =============================================================================================
// vaw_gemm: validate -> plan -> launch.  Every choice -- kernel, tile, split, grid, LDS, which passes follow -- is made by
// vaw_gemm_plan (gemm_plan.hip); the code below only carries it out.
// =============================================================================================
static_assert(FastCfg<32>::lds_bytes == vaw_lds_t128(32) && FastCfg<64>::lds_bytes == vaw_lds_t128(64) && BIG_LDS == vaw_lds_ring256() &&
              2 * GBK * GLD * 4 == vaw_lds_generic(), "gemm_plan.h: LDS sizes of the kernels in this file");

// launchers of the other translation units: the tile parameters, epilogue kind and grid are the plan's
void vaw_sm_launch(int mb, int nb, int stages, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda,
                   const bf16_t* b, int64_t ldb, const EpiDev& e, hipStream_t s);      // gemm_sm.hip
void vaw_p8_conv(const vaw_conv3x3_launch& p, int mode, const bf16_t* act, const bf16_t* act2, const bf16_t* w, void* out, int H, int W,
                 int Ci, int Co, EpiDev e, float* workspace, hipStream_t s, float* bias_grad, float bias_beta);
void vaw_p8_launch(const P8Plan& pl, int epi, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda,
                   const bf16_t* b, int64_t ldb, const EpiDev& e, hipStream_t s);
void vaw_pd_launch(int ntw, int epi, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda, const bf16_t* b,
                   int64_t ldb, const EpiDev& e, int grid, hipStream_t s);
void vaw_ws_launch(int ntw, int epi, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a, int64_t lda, const bf16_t* b,
                   int64_t ldb, const EpiDev& e, int grid, bool loaders8, hipStream_t s);

// the fixed-order pass over the split-K slabs (reduce: vaw_gemm_reduce; rowpart / rowsum_out: VAW_GR_F32_ROWSUM and conv3x3 mode 2)
static void splitk_reduce(int reduce, const float* slab, int split, int64_t M, int64_t N, int64_t ldc, void* C, float alpha, float beta,
                          hipStream_t s, const float* rowpart = nullptr, float* rowsum_out = nullptr, float rowsum_beta = 0.f) {
    const int grid = ceil_div(M * N / 4, 256) > 2048 ? 2048 : ceil_div(M * N / 4, 256);
    if (reduce == VAW_GR_BF16) splitk_reduce_kernel<bf16_t><<<grid, 256, 0, s>>>(slab, split, M, N, ldc, C, alpha, 0.f, 0);
    else splitk_reduce_kernel<float><<<grid, 256, 0, s>>>(slab, split, M, N, ldc, C, alpha, beta, 1, rowpart, rowsum_out, rowsum_beta);
}

// A kernel has one instantiation per operand layout, tabled as [a_kmajor][b_kmajor]; each raises its dynamic-LDS cap on first use.
template <typename Fn>
static Fn by_layout(Fn const (&tab)[2][2], bool (&raised)[2][2], int a_kmajor, int b_kmajor, int lds) {
    const int ak = a_kmajor != 0, bk = b_kmajor != 0;
    if (lds > 0 && !raised[ak][bk]) {
        (void)hipFuncSetAttribute((const void*)tab[ak][bk], hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        raised[ak][bk] = true;
    }
    return tab[ak][bk];
}
#define LAYOUT_TABLE(KERNEL, ...) \
    {{KERNEL<false, false, ##__VA_ARGS__>, KERNEL<false, true, ##__VA_ARGS__>}, {KERNEL<true, false, ##__VA_ARGS__>, KERNEL<true, true, ##__VA_ARGS__>}}

template <int BKT>
static void launch_t128(const vaw_gemm_launch& p, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a,
                        int64_t lda, const bf16_t* b, int64_t ldb, const EpiDev& e, hipStream_t s) {
    using Fn = decltype(&gemm_bf16_kernel<true, true, BKT, 0>);
    static const Fn tab[2][2] = LAYOUT_TABLE(gemm_bf16_kernel, BKT, 0);
    static bool raised[2][2];
    const int tiles_n = (int)((N + BN - 1) / BN), n_wg = (int)((M + BM - 1) / BM) * tiles_n;
    by_layout(tab, raised, a_kmajor, b_kmajor, (int)p.lds_bytes)<<<dim3(p.grid_x, p.grid_y), p.block, p.lds_bytes, s>>>(
        a, lda, b, ldb, (int)(K / BKT), tiles_n, n_wg, p.split, e, ConvGeom{}, p.xcd_parts);
}
static void launch_ring256(const vaw_gemm_launch& p, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, const bf16_t* a,
                           int64_t lda, const bf16_t* b, int64_t ldb, const EpiDev& e, hipStream_t s) {
    using Fn = decltype(&gemm_bf16_big_kernel<true, true>);
    static const Fn tab[2][2] = LAYOUT_TABLE(gemm_bf16_big_kernel);
    static bool raised[2][2];
    const int tiles_n = (int)((N + BIG_BN - 1) / BIG_BN), n_wg = (int)((M + BIG_BM - 1) / BIG_BM) * tiles_n;
    by_layout(tab, raised, a_kmajor, b_kmajor, (int)p.lds_bytes)<<<dim3(p.grid_x, p.grid_y), p.block, p.lds_bytes, s>>>(
        a, lda, b, ldb, (int)(K / p.bkt), tiles_n, n_wg, p.split, e);
}
template <typename T>
static void launch_generic(const vaw_gemm_launch& p, int a_kmajor, int b_kmajor, int64_t K, const void* A, int64_t lda, const void* B,
                           int64_t ldb, const EpiDev& e, hipStream_t s) {
    using Fn = decltype(&gemm_generic_kernel<T, true, true>);
    static const Fn tab[2][2] = {{gemm_generic_kernel<T, false, false>, gemm_generic_kernel<T, false, true>},
                                 {gemm_generic_kernel<T, true, false>, gemm_generic_kernel<T, true, true>}};
    static bool raised[2][2];
    const int64_t kchunk = p.split > 1 ? ((K + p.split - 1) / p.split + GBK - 1) / GBK * GBK : K;     // (splits of whole GBK steps)
    by_layout(tab, raised, a_kmajor, b_kmajor, 0)<<<dim3(p.grid_x, p.grid_y, p.grid_z), p.block, 0, s>>>(
        (const T*)A, lda, (const T*)B, ldb, K, kchunk, e);
}

extern "C" int vaw_gemm(vaw_dtype dt, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, const void* A,
                        int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const vaw_epilogue* ep,
                        float* workspace, int64_t workspace_floats, vaw_stream stream) {
    vaw_gemm_launch p;
    int rc = vaw_gemm_plan(dt, a_kmajor, b_kmajor, M, N, K, lda, ldb, ldc, (int64_t)(uintptr_t)A, (int64_t)(uintptr_t)B,
                           (int64_t)(uintptr_t)C, ep, workspace ? workspace_floats : 0, nullptr, &p);
    if (rc) return rc;         // (every refusal: nothing has been launched)
    const GemmKnobs& k = vaw_gemm_knobs_state();
    EpiDev e = vaw_epi_dev(ep, k);
    if (dt == VAW_F32) e.out_f32 = 1;
    e.M = M; e.N = N; e.ldc = ldc; e.C = C; e.slab = workspace;
    // column sums: the kernel leaves partial rows in the workspace (folded below) or with the caller (colsum_partial_out)
    if (p.colsum_mode == VAW_GC_FOLD) e.colpart = workspace;
    if (p.colsum_mode == VAW_GC_DEFERRED) e.colpart = ep->colsum_partial_out;
    if (p.rowsum_mode == VAW_GS_FUSED) e.rowpart = workspace + (p.split > 1 ? (int64_t)p.split * M * N : 0);      // behind the slabs
    const bf16_t* a = (const bf16_t*)A;
    const bf16_t* b = (const bf16_t*)B;
    hipStream_t s = (hipStream_t)stream;
    switch (p.variant) {
        case VAW_GV_SMALL_M: vaw_sm_launch(p.mb, p.nb, p.stages, b_kmajor, M, N, K, a, lda, b, ldb, e, s); break;
        case VAW_GV_PARKED_DRAIN:
        case VAW_GV_WARP_SPEC: {
            EpiDev ed = e;
            ed.nt_off = 1, ed.nt_aux = k.nt_aux;
            if (p.variant == VAW_GV_WARP_SPEC) vaw_ws_launch(p.ntw, p.epi_kind, b_kmajor, M, N, K, a, lda, b, ldb, ed, p.grid_x, p.block == 1024, s);
            else vaw_pd_launch(p.ntw, p.epi_kind, b_kmajor, M, N, K, a, lda, b, ldb, ed, p.grid_x, s);
            break;
        }
        case VAW_GV_PERSISTENT: {
            // default cache policy for the epilogue stores (nt costs 5-15 % on the f32 gated-residual and 192-column launches, and the
            // next kernel re-reads the output from L2 / MALL); the aux_out stores alone are non-temporal (-0.5 % on the DiT-B/4 step)
            EpiDev e8 = e;
            e8.nt_off = !k.p8_nt, e8.nt_aux = k.nt_aux;
            vaw_p8_launch(P8Plan{true, p.ntw, p.split, p.grid_x}, p.epi_kind, a_kmajor, b_kmajor, M, N, K, a, lda, b, ldb, e8, s);
            break;
        }
        case VAW_GV_RING256: launch_ring256(p, a_kmajor, b_kmajor, M, N, K, a, lda, b, ldb, e, s); break;
        case VAW_GV_T128_BK32: launch_t128<32>(p, a_kmajor, b_kmajor, M, N, K, a, lda, b, ldb, e, s); break;
        case VAW_GV_T128_BK64: launch_t128<64>(p, a_kmajor, b_kmajor, M, N, K, a, lda, b, ldb, e, s); break;
        default:
            if (dt == VAW_F32) launch_generic<float>(p, a_kmajor, b_kmajor, K, A, lda, B, ldb, e, s);
            else launch_generic<bf16_t>(p, a_kmajor, b_kmajor, K, A, lda, B, ldb, e, s);
            break;
    }
    float* const rowsum_out = ep ? ep->rowsum_a_out : nullptr;
    if (p.reduce != VAW_GR_NONE)
        splitk_reduce(p.reduce, workspace, p.split, M, N, ldc, C, e.alpha, e.beta, s, e.rowpart, rowsum_out, ep ? ep->rowsum_a_beta : 0.f);
    VAW_CHECK_LAUNCH("gemm");
    // the fold of the column-sum rows goes first: a separate row-sum pass reuses the workspace they lie in
    if (p.colsum_mode == VAW_GC_FOLD && (rc = vaw_reduce_rows(workspace, p.colsum_rows, N, ep->colsum_out, ep->colsum_beta, stream))) return rc;
    // row sums of A: the MFMA kernel's partials (folded by the reduce when there was one), or, A being stored [K][M], a column sum over its K rows
    if (p.rowsum_mode == VAW_GS_FUSED && p.reduce == VAW_GR_NONE) rc = vaw_reduce_rows(e.rowpart, 1, M, rowsum_out, ep->rowsum_a_beta, stream);
    else if (p.rowsum_mode == VAW_GS_SEPARATE) rc = vaw_colsum(dt, A, K, M, lda, rowsum_out, ep->rowsum_a_beta, workspace, workspace_floats, stream);
    if (rc) return rc;
    switch (p.colsum_mode) {
        case VAW_GC_DEFERRED: *ep->colsum_rows_out = p.colsum_rows; return VAW_OK;
        case VAW_GC_SEPARATE:      // a pass over the output just written; deferred: its one complete row is the only "partial" row
            if (ep->colsum_partial_out) *ep->colsum_rows_out = p.colsum_rows;
            return vaw_colsum(e.out_f32 ? VAW_F32 : dt, C, M, N, ldc, ep->colsum_partial_out ? ep->colsum_partial_out : ep->colsum_out,
                              ep->colsum_partial_out ? 0.f : ep->colsum_beta, workspace, workspace_floats, stream);
        default: return VAW_OK;
    }
}


// =============================================================================================
// conv3x3 (stride 1, pad 1, NHWC) as implicit GEMM on the MFMA kernel.  Returns VAW_ERR_UNSUPPORTED when the
// shape needs the explicit path (f32 parity mode, channel counts that are not multiples of 64, ...).
//   mode 0  y[M,Co]   = conv(x; W) (+ epilogue)          act = x  [M,Ci]
//   mode 1  dx[M,Ci]  = conv^T(dy; W)                    act = dy [M,Co]
//   mode 2  dW[Co,9Ci] (f32) = beta*dW + dy^T . patches(x)   act = dy, act2 = x
// W is stored [Co][3][3][Ci] (channels-last), act dtype.
// =============================================================================================
extern "C" int vaw_conv3x3(vaw_dtype dt, int mode, const void* act, const void* act2, const void* w, void* out, int B, int H,
                           int W, int Ci, int Co, const vaw_epilogue* ep, float* workspace, int64_t workspace_floats,
                           vaw_stream stream) {
    // validate -> plan -> launch: every check and choice is vaw_conv3x3_plan's (gemm_plan.hip); the code below only carries it out
    vaw_conv3x3_launch p;
    int rc = vaw_conv3x3_plan(dt, mode, (int64_t)(uintptr_t)act, (int64_t)(uintptr_t)act2, (int64_t)(uintptr_t)w, (int64_t)(uintptr_t)out, B, H,
                              W, Ci, Co, ep, (int64_t)(uintptr_t)workspace, workspace_floats, nullptr, 0, &p);
    if (rc) return rc;         // (every refusal: nothing has been launched)
    EpiDev e = vaw_epi_dev(ep, vaw_gemm_knobs_state());
    e.debug = 0;            // (the ablation switch of VAW_GEMM_DEBUG belongs to vaw_gemm's launches)
    if (mode == 2) e.out_f32 = 1;
    const int64_t Mpix = (int64_t)B * H * W, M = p.M, N = p.N;
    e.M = M; e.N = N; e.ldc = N; e.C = out; e.slab = workspace;
    float* const rowsum_out = ep ? ep->rowsum_a_out : nullptr;
    const float rowsum_beta = ep ? ep->rowsum_a_beta : 0.f;
    hipStream_t s = (hipStream_t)stream;
    if (p.variant == VAW_GV_PERSISTENT) {      // gemm_p8_conv.hip
        vaw_p8_conv(p, mode, (const bf16_t*)act, (const bf16_t*)act2, (const bf16_t*)w, out, H, W, Ci, Co, e, workspace, s, rowsum_out, rowsum_beta);
        VAW_CHECK_LAUNCH("conv3x3_p8");
        if (p.bias_grad == VAW_CVB_SEPARATE)     // bias gradient = column sums of dy [Mpix][Co], as a pass of its own
            return vaw_colsum(dt, act, Mpix, Co, Co, rowsum_out, rowsum_beta, workspace, workspace_floats, stream);
        return VAW_OK;
    }
    const int tiles_n = (int)((N + BN - 1) / BN);
    const int n_wg = (int)((M + BM - 1) / BM) * tiles_n;
    const int nk_total = (int)(p.K / 64);
    if (p.colsum_mode == VAW_GC_FOLD) e.colpart = workspace;
    float* rowpart = nullptr;
    if (p.bias_grad != VAW_CVB_NONE) rowpart = e.rowpart = workspace + (p.split > 1 ? (int64_t)p.split * M * N : 0);     // behind the slabs
    const dim3 grid((unsigned)p.grid_x, (unsigned)p.grid_y);
    const ConvGeom cg{H, W, Ci, Co};
    const int lds = (int)p.lds_bytes;
#define LAUNCH_CONV(AKv, BKv, CV, Aptr, LDA, Bptr, LDB)                                                                  \
    do {                                                                                                                 \
        static bool attr_done = false;                                                                                   \
        if (!attr_done) {                                                                                                \
            (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<AKv, BKv, 64, CV>,                                   \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds);                                  \
            attr_done = true;                                                                                            \
        }                                                                                                                \
        gemm_bf16_kernel<AKv, BKv, 64, CV><<<grid, p.block, lds, s>>>((const bf16_t*)(Aptr), LDA, (const bf16_t*)(Bptr), LDB, \
                                                                      nk_total, tiles_n, n_wg, p.split, e, cg, p.xcd_parts); \
    } while (0)
    if (mode == 0) LAUNCH_CONV(true, true, 1, act, (int64_t)Ci, w, 9LL * Ci);
    else if (mode == 1) LAUNCH_CONV(true, false, 2, act, (int64_t)Co, w, 9LL * Ci);
    else LAUNCH_CONV(false, false, 3, act, (int64_t)Co, act2, (int64_t)Ci);
    if (p.reduce != VAW_CVR_NONE) splitk_reduce(VAW_GR_F32, workspace, p.split, M, N, N, out, e.alpha, e.beta, s, rowpart, rowsum_out, rowsum_beta);
    VAW_CHECK_LAUNCH("conv3x3");
    if (p.bias_grad == VAW_CVB_FOLD) return vaw_reduce_rows(rowpart, 1, M, rowsum_out, rowsum_beta, stream);
    if (p.colsum_mode == VAW_GC_FOLD) return vaw_reduce_rows(workspace, p.colsum_rows, N, ep->colsum_out, ep->colsum_beta, stream);
    return VAW_OK;
}

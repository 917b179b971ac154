// Four-wave engine for the bf16 grouped weight gradient dW_p (+)= dy_p^T x_p (vaw_wgrad_grouped, 256-column tiles).
//
// The same GEMM as gemm_p8_kernel<false, false, 4, P8_WGRAD, true> (gemm_p8_kernel.h), and bitwise the same results: the same
// 256 x 256 x 64 tile, the same v_mfma_f32_16x16x32_bf16, the same K order and K-split points, the same item list (P8Prob / P8Group:
// whole tiles, then the K-split tiles of the last partial round), XCD item mapping, slab layout, LDS images (P8_PART, p8_src_off,
// p8_mn_swz) and epilogue arithmetic -- every output element sees the same sequence of MFMA accumulations.  What differs is who does it:
//   * 256 threads, ONE wave per SIMD, waves 2 (M) x 2 (N), wave tile 128 x 128 = 8 x 8 accumulator tiles (256 registers; the wave owns
//     its SIMD's whole 512-entry file).  Per K tile the four waves read 4 x (128 + 128) x 64 x 2 B = 128 KB of fragments where the
//     eight 128 x 64 waves read 192 KB;
//   * the K loop is one software pipeline over HALF K tiles (32 of K: 8 A + 8 B fragments = 64 registers, 64 MFMAs per wave).  While
//     the MFMAs of one half issue (row i = A fragment i against the 8 B fragments), the 16 fragments of the next half are read into
//     the other fragment buffer, two per row, and one LDS-DMA piece per row goes out, all between the MFMAs of that row.  Fragment
//     reads are waited for with counted s_waitcnt lgkmcnt(14 / 15) (LDS operations of a wave return in order; a count below the number
//     of reads issued behind the one needed is safe, scalar loads in flight only make it stricter), DMA pieces with vmcnt(8);
//   * LDS: two 64 KiB stages as in gemm_p8_kernel, handed over in halves.  An 8 KiB part is 8 pieces of 1 KiB (8 k rows each); wave w
//     issues pieces w (k 0-31, sub-stage 0) and 4 + w (k 32-63, sub-stage 1) of every part, so a half K tile is 8 pieces per wave.
//     The four sub-stages form a ring: while half q computes, the fragments of half q + 1 are read and the pieces of half q + 3 are
//     issued into the sub-stage that half q - 1 was read from.  ONE workgroup barrier per half, at its end, behind vmcnt(8): it says
//     both "every wave's pieces of half q + 2 have landed" and "every wave has its fragments of half q in registers" (the last row's
//     wait covers them), which is what the issue of half q + 4's pieces and the reads of half q + 2 in the next half need;
//   * the ring and the fragment pipeline run on across item boundaries: the last half of an item reads the first fragments of the
//     next one, whose first three halves are in LDS or in flight during the epilogue;
//   * epilogue through the wave-private 4 KiB LDS image of gemm_p8_kernel, once per 64-column half of the wave tile.
#pragma once
#include "gemm_p8_kernel.h"

#define G4_STAGE (8 * P8_PART)                  // 4 A parts + 4 B parts
#define G4_EPI_BYTES (4 * 4096)                 // one image per wave
#define G4_LDS_BYTES (2 * G4_STAGE + G4_EPI_BYTES)
static_assert(G4_STAGE == P8Cfg<4>::stage_bytes, "the stage layout of gemm_p8_kernel");
static_assert(G4_LDS_BYTES <= 160 * 1024, "LDS of one CU");
static_assert(7 * P8_PART + 4096 + 512 < 65536, "fragment reads address a whole stage through the 16-bit DS offset");

// 16 x 32 mn-major operand fragment at a per-lane address (p8_frag<false> with the part, the k sub-step and the stage in OFF / addr)
template <int OFF>
__device__ __forceinline__ bf16x8 g4_frag(unsigned addr) {
    bf16x4 lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
                 : "=&v"(lo), "=&v"(hi)
                 : "v"(addr), "i"(OFF), "i"(OFF + 512)
                 : "memory");
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

#define G4_SB() __builtin_amdgcn_sched_barrier(0)
#define G4_IC(v) std::integral_constant<int, (v)>{}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
gemm_g4_kernel(int nk_total, EpiDev e, const P8Prob* __restrict__ probs, P8Group grp) {
    constexpr int BN = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][A parts 0-3 | B parts 0-3] | 4 x 4 KiB epilogue images
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    // ---- static item list, as in gemm_p8_kernel ----
    const int G = gridDim.x;
    const int n_items = grp.t_full + grp.t_rem * grp.n_split;
    int it_cur;
    {
        const int b = blockIdx.x, x = b & 7, q = G >> 3, r = G & 7;
        it_cur = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
    }
    if (it_cur >= n_items) return;
    const int nk_per = (nk_total + grp.n_split - 1) / grp.n_split;
    auto decode = [&](int it) __attribute__((always_inline)) {
        P8Item t;
        int g;
        if (it < grp.t_full) { g = it; t.split = -1; t.rem = 0; t.kt0 = 0; t.nk = nk_total; }
        else {
            const int j = it - grp.t_full;
            t.split = j / grp.t_rem;
            t.rem = j - t.split * grp.t_rem;
            g = grp.t_full + t.rem;
            t.kt0 = t.split * nk_per;
            t.nk = t.kt0 + nk_per <= nk_total ? nk_per : nk_total - t.kt0;
        }
        int pi = 0;
        while (pi + 1 < grp.n_prob && probs[pi + 1].tile0 <= g) ++pi;      // uniform: scalar loads
        const P8Prob& pr = probs[pi];
        const int tile = g - pr.tile0, tm = tile / pr.tiles_n;
        t.prob = pi; t.tm = tm;
        t.a = pr.a; t.b = pr.b; t.lda = pr.lda; t.ldb = pr.ldb; t.M = pr.M; t.N = pr.N;
        t.m0 = (int64_t)tm * P8_BM;
        t.n0 = (int64_t)(tile - tm * pr.tiles_n) * BN;
        return t;
    };

    // ---- the DMA stream: its own item / K-tile position, three halves ahead of the MFMAs ----
    int iss_item = it_cur, iss_kt = 0, iss_nk = 0, iss_stage = 0;
    bool iss_done = false;
    __amdgpu_buffer_rsrc_t rs_a = epi_rsrc(probs), rs_b = epi_rsrc(probs);
    unsigned so_a = 0, so_b = 0, step_a = 0, step_b = 0;
    u32x4_t off_a = {0, 0, 0, 0}, off_b = {0, 0, 0, 0};     // piece `wid` of each part; piece 4 + wid lies 32 k rows = half a step further on
                                                            // (vectors, not arrays: values the optimiser keeps out of private memory)
    auto iss_open = [&]() __attribute__((always_inline)) {
        const P8Item t = decode(iss_item);
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));        // opaque per item: the per-lane parts of the offsets are rebuilt here, not kept live
        iss_nk = t.nk;
        iss_kt = 0;
        const int mvalid = t.M - t.m0 < P8_BM ? (int)(t.M - t.m0) : P8_BM;
        const int nvalid = t.N - t.n0 < BN ? (int)(t.N - t.n0) : BN;
        step_a = (unsigned)(64 * t.lda * 2);
        step_b = (unsigned)(64 * t.ldb * 2);
        so_a = so_b = 0;
        rs_a = epi_rsrc((const char*)t.a + (t.m0 + t.kt0 * 64 * t.lda) * 2);
        rs_b = epi_rsrc((const char*)t.b + (t.n0 + t.kt0 * 64 * t.ldb) * 2);
        off_a = u32x4_t{p8_src_off<false>(true, 0, wid, lane, t.lda, mvalid), p8_src_off<false>(true, 1, wid, lane, t.lda, mvalid),
                        p8_src_off<false>(true, 2, wid, lane, t.lda, mvalid), p8_src_off<false>(true, 3, wid, lane, t.lda, mvalid)};
        off_b = u32x4_t{p8_src_off<false>(false, 0, wid, lane, t.ldb, nvalid), p8_src_off<false>(false, 1, wid, lane, t.ldb, nvalid),
                        p8_src_off<false>(false, 2, wid, lane, t.ldb, nvalid), p8_src_off<false>(false, 3, wid, lane, t.ldb, nvalid)};
    };
    auto iss_close = [&]() __attribute__((always_inline)) {                      // past the last item every piece reads out of range: zeros into a stage nobody reads
        off_a = off_b = u32x4_t{EPI_OOB, EPI_OOB, EPI_OOB, EPI_OOB};
    };
    // piece c (B parts 0-3, then A parts 0-3) of sub-stage SUB of the stream's K tile
    auto iss_piece = [&](auto cc, auto subc) __attribute__((always_inline)) {
        constexpr int c = decltype(cc)::value, sub = decltype(subc)::value;
        char* dst = smem + iss_stage * G4_STAGE + (4 * sub + wid) * 1024;
        if constexpr (c < 4) p8_dma16(rs_b, dst + 4 * P8_PART + c * P8_PART, off_b[c], __builtin_amdgcn_readfirstlane(so_b + sub * (step_b >> 1)));
        else p8_dma16(rs_a, dst + (c - 4) * P8_PART, off_a[c - 4], __builtin_amdgcn_readfirstlane(so_a + sub * (step_a >> 1)));
    };
    auto iss_advance = [&]() __attribute__((always_inline)) {                    // after the last piece of a K tile
        iss_stage ^= 1;
        if (iss_done) return;
        so_a += step_a;
        so_b += step_b;
        if (++iss_kt == iss_nk) {
            iss_item += G;
            if (iss_item >= n_items) { iss_done = true; iss_close(); }
            else iss_open();
        }
    };
#define G4_PIECES(SUB)                                                                                                       \
    do {                                                                                                                     \
        iss_piece(G4_IC(0), G4_IC(SUB)); iss_piece(G4_IC(1), G4_IC(SUB)); iss_piece(G4_IC(2), G4_IC(SUB)); iss_piece(G4_IC(3), G4_IC(SUB)); \
        iss_piece(G4_IC(4), G4_IC(SUB)); iss_piece(G4_IC(5), G4_IC(SUB)); iss_piece(G4_IC(6), G4_IC(SUB)); iss_piece(G4_IC(7), G4_IC(SUB)); \
    } while (0)

    // ---- fragment addresses (p8_frag<false>): per lane, one per 16-row group of a part; the swizzle depends on the lane alone ----
    unsigned rA[2], rB[4];
    {
        const int li = lane & 15, q = li >> 2, p = li & 3;
        const int kb0 = 8 * (lane >> 4) + q, swz = p8_mn_swz(kb0);
        const unsigned lane_off = (unsigned)(uintptr_t)(lds_ptr_t)smem + kb0 * 128 + ((p >> 1) << 4) + 8 * (p & 1);
#pragma unroll
        for (int t = 0; t < 2; ++t) rA[t] = lane_off + (((4 * wr + 2 * t) ^ swz) << 4);                       // rows 32 wr + 16 t of an A part
#pragma unroll
        for (int k = 0; k < 4; ++k) rB[k] = lane_off + 4 * P8_PART + 2 * wc * P8_PART + (((2 * k) ^ swz) << 4);   // B parts 2 wc, 2 wc + 1
    }
    int rd_delta = G4_STAGE;                      // the stage the fragment reads are on alternates per K tile
    bf16x8 fa[2][8], fb[2][8];                    // [k half][fragment]: A rows 16 i of the wave tile, B columns 16 u
    auto read_frag = [&](auto nxc, auto fc) __attribute__((always_inline)) {     // fragment f of k half nx: 0-7 B, 8-15 A
        constexpr int nx = decltype(nxc)::value, f = decltype(fc)::value;
        if constexpr (f < 8) fb[nx][f] = g4_frag<(f >> 2) * P8_PART + nx * 4096>(rB[f & 3]);
        else fa[nx][f - 8] = g4_frag<((f - 8) >> 1) * P8_PART + nx * 4096>(rA[(f - 8) & 1]);
    };

    // prologue: three halves of the stream; the first two landed; the fragments of the first half
    iss_open();
    G4_PIECES(0);
    G4_PIECES(1);
    iss_advance();
    G4_PIECES(0);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    G4_SB();
    read_frag(G4_IC(0), G4_IC(0)); read_frag(G4_IC(0), G4_IC(1)); read_frag(G4_IC(0), G4_IC(2)); read_frag(G4_IC(0), G4_IC(3));
    read_frag(G4_IC(0), G4_IC(4)); read_frag(G4_IC(0), G4_IC(5)); read_frag(G4_IC(0), G4_IC(6)); read_frag(G4_IC(0), G4_IC(7));
    read_frag(G4_IC(0), G4_IC(8)); read_frag(G4_IC(0), G4_IC(9)); read_frag(G4_IC(0), G4_IC(10)); read_frag(G4_IC(0), G4_IC(11));
    read_frag(G4_IC(0), G4_IC(12)); read_frag(G4_IC(0), G4_IC(13)); read_frag(G4_IC(0), G4_IC(14)); read_frag(G4_IC(0), G4_IC(15));
    G4_SB();

    for (; it_cur < n_items; it_cur += G) {
        const P8Item item = decode(it_cur);
        const int split = item.split, nk = item.nk;
        const int64_t m0 = item.m0, n0 = item.n0;
        f32x4 acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[i][u] = f32x4{0, 0, 0, 0};
        // row i of k half s: 8 MFMAs; between them two fragments of the next half and one DMA piece.  Reads issued behind A fragment i
        // of this half when the wait stands: 2 (7 - i) of its own half + 4 i of the next, >= 15 from row 1 on and 14 in row 0 (which
        // also needs the B fragments, all older).
        auto row = [&](auto sc, auto ic) __attribute__((always_inline)) {
            constexpr int s = decltype(sc)::value, i = decltype(ic)::value, nx = s ^ 1;
            if constexpr (i == 0) asm volatile("s_waitcnt lgkmcnt(14)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory");
            G4_SB();
#define G4_MMA(u) acc[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[s][u], fa[s][i], acc[i][u], 0, 0, 0)
            G4_MMA(0);
            G4_SB();
            read_frag(G4_IC(nx), G4_IC(2 * i));
            G4_SB();
            G4_MMA(1);
            G4_MMA(2);
            G4_SB();
            read_frag(G4_IC(nx), G4_IC(2 * i + 1));
            G4_SB();
            G4_MMA(3);
            G4_MMA(4);
            G4_SB();
            iss_piece(G4_IC(i), G4_IC(nx));
            G4_SB();
            G4_MMA(5);
            G4_MMA(6);
            G4_MMA(7);
#undef G4_MMA
            G4_SB();
        };
#define G4_HALF(S)                                                                                                           \
    do {                                                                                                                     \
        row(G4_IC(S), G4_IC(0)); row(G4_IC(S), G4_IC(1)); row(G4_IC(S), G4_IC(2)); row(G4_IC(S), G4_IC(3));                  \
        row(G4_IC(S), G4_IC(4)); row(G4_IC(S), G4_IC(5)); row(G4_IC(S), G4_IC(6)); row(G4_IC(S), G4_IC(7));                  \
    } while (0)
        for (int kt = 0; kt < nk; ++kt) {
            // k half 0: reads k half 1 of this K tile, issues k half 1 of the stream's K tile (one ahead), then moves the stream on
            G4_HALF(0);
            iss_advance();
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            G4_SB();
            // k half 1: reads k half 0 of the next K tile (the other stage), issues k half 0 of the stream's K tile (two ahead)
#pragma unroll
            for (int t = 0; t < 2; ++t) rA[t] += rd_delta;
#pragma unroll
            for (int k = 0; k < 4; ++k) rB[k] += rd_delta;
            rd_delta = -rd_delta;
            G4_HALF(1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            G4_SB();
        }
#undef G4_HALF
        // the fragments of the next item's first half are in flight: landed before the epilogue's code may touch their registers
        // (and the last MFMAs' results written: the epilogue's inline-asm stores read the accumulators, a hazard the compiler does not pad)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15" ::: "memory");
        G4_SB();

        // ---- epilogue (gemm_p8_kernel's, P8_WGRAD): per 64-column half, 8 row tiles of 16 rows through the wave's LDS image ----
        const P8Prob& pr = probs[item.prob];
        EpiDev ei{};                          // (built field by field: a copy of the kernel argument stays in private memory)
        ei.beta = e.beta; ei.nt_off = 1; ei.out_f32 = 1; ei.rpb = 1;      // (nt_off: what vaw_wgrad_grouped sets, default cache policy)
        ei.C = pr.c; ei.ldc = pr.ldc; ei.M = pr.M; ei.N = pr.N; ei.alpha = pr.alpha;
        char* ep = smem + 2 * G4_STAGE + wid * 4096;
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));      // opaque per item: the epilogue's per-lane addresses are not kept across the K loop
        const int wr_row = lane_e & 15, wr_g = lane_e >> 4;             // accumulator layout: row, group of 4 columns
        const int rd_row = lane_e >> 3, rd_c8 = lane_e & 7;             // read-back layout: row within 8, group of 8 columns
        // 16-byte chunk c of row r lives at r * 256 + ((c ^ r) << 4); written and read with inline-asm DS instructions (an ordinary
        // LDS access beside pending LDS-DMA makes the compiler drain vmcnt); DS operations of one wave execute in order
        const unsigned ep_base = (unsigned)(uintptr_t)(lds_ptr_t)ep;
        const unsigned ep_w = ep_base + wr_row * 256 + ((wr_g ^ (wr_row & 3)) << 4);
        unsigned ep_r[2];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int rr = pass * 8 + rd_row;
            ep_r[pass] = ep_base + rr * 256 + (((2 * rd_c8) ^ rr) << 4);     // chunk 2c; chunk 2c + 1 is this address ^ 16
        }
        const int64_t m_last = ei.M - 1;
        const int64_t tile_off = m0 * ei.ldc + n0;
        const bool to_slab = split >= 0;      // K-split items: raw partial sums into slabs [split][tile][256][256]
        const __amdgpu_buffer_rsrc_t rs_c =
            to_slab ? epi_rsrc(grp.slab + ((int64_t)split * grp.t_rem + item.rem) * (P8_BM * BN)) : epi_rsrc((const float*)ei.C + tile_off);
        const int64_t mrow0 = m0 + wr * 128 + rd_row;
        const f32x4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
        const EpiOps no_ops{};
        float qmax = 0.f;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int wn0 = wc * 128 + 64 * hh;
            const int64_t n = n0 + wn0 + 8 * rd_c8;
            const bool col_ok = n < ei.N;                                    // N % 8 == 0: a group is in or out as a whole
            const int64_t n_ld = col_ok ? n : n0;
            const int loc_col = wn0 + 8 * rd_c8;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    asm volatile("ds_write_b128 %0, %1" ::"v"(ep_w + (unsigned)(((4 * u) ^ (wr_row & 12)) << 4)), "a"(acc[i][4 * hh + u]) : "memory");
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const int k = 2 * i + pass;
                    const int64_t m = mrow0 + 8 * k;
                    f32x4 v0, v1;
                    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(v0), "=&v"(v1)
                                 : "v"(ep_r[pass]), "v"(ep_r[pass] ^ 16u)
                                 : "memory");
                    G4_SB();                         // nothing that reads v0 / v1 may move above the wait
                    const bool ok = col_ok && m <= m_last;
                    const int loc = ok ? (int)((m - m0) * ei.ldc) + loc_col : -1;
                    if (to_slab) {
                        const unsigned bo = ok ? 4u * (unsigned)((m - m0) * BN + loc_col) : EPI_OOB;
                        buf_store16(rs_c, bo, v0, false);
                        buf_store16(rs_c, ok ? bo + 16u : EPI_OOB, v1, false);
                    } else {
                        const int64_t mc = m <= m_last ? m : m_last;
                        epi_apply8<P8_WGRAD>(ei, rs_c, rs_c, loc, (const float*)ei.C + mc * ei.ldc + n_ld, v0, v1, b0, b1, no_ops, qmax);
                    }
                    G4_SB();                         // keep the unrolled steps apart
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // the stream's trailing pieces still target this workgroup's LDS
#undef G4_PIECES
}

static void g4_launch_group(int nk, int grid, const EpiDev& e, const P8Prob* probs_dev, const P8Group& grp, hipStream_t s) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_g4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, G4_LDS_BYTES);
        attr_done = true;
    }
    gemm_g4_kernel<<<grid, 256, G4_LDS_BYTES, s>>>(nk, e, probs_dev, grp);
}

// Evaluation metrics from activations (evaluations/evaluator.py of the reference): the all-pairs squared distances of
// ManifoldEstimator with their selection fused into the tile epilogue, and the float64 mean / covariance of FIDStatistics.
//
// Built with -ffp-contract=off: the epilogue arithmetic is the expression as written, every operation rounded on its own.
//
// Pairwise kernels.  One 256-thread block owns a 128-row tile of U and walks a range of 128-row tiles of V.  The product
// U_i . V_j runs on v_mfma_f32_32x32x2_f32 (exact f32 inputs, the result a k-ordered fmaf chain): every output element walks
// k = 0 .. D-1 in order in ONE accumulator, K is never split, the zero padding past D only appends fma(0, 0, acc) = acc.  A
// distance therefore has the same bits whatever tile, block or launch computed it, which is what makes the results independent
// of every chunking above.  The 128 x 128 distances never leave the CU: they are staged through LDS in two 128 x 64 halves and
// consumed there (a sorted k-list per thread, the radius comparisons or their counts).  The polynomial-kernel row sums of the kernel
// inception distance stage the dot products themselves and add (gamma dot + coef0)^degree per row in float64 in a fixed order;
// their operands may be read through index tables (pw_product_of with PwGatheredRows).
//
// Inception score.  The head product logits = X Wt^T is the same tile (pw_product, one block per 128 x 128 output tile, the
// accumulators stored straight to memory); the softmax, the entropies and the class marginals are float64 sums in a fixed order.
#include <math.h>

#include "common.h"

namespace {

constexpr int PW_T = 128;        // tile rows of U and of V
constexpr int PW_BK = 16;        // k per staged slab
constexpr int PW_LD = 132;       // floats per k row of a staged operand slab ([k][row], 4 floats of padding)
constexpr int PW_DLD = 65;       // floats per row of the staged half tile of distances
constexpr int PW_SPLITS = 16;    // most column ranges one row tile is cut into
constexpr int PW_KMAX = 16;      // largest k1
constexpr int PW_RMAX = 4;       // most radii per point

struct PwShared {
    float a[PW_BK * PW_LD];
    float b[PW_BK * PW_LD];
    float d[PW_T * PW_DLD];
    float nu[PW_T], nv[PW_T];
    float ru[PW_T * PW_RMAX], rv[PW_T * PW_RMAX];
};
static_assert(sizeof(PwShared) <= 65536, "static LDS");

// rows row0 + (t >> 4) + 16 p, column k0 + (t & 15): 64-byte runs along k, zeros past the last row and past D
__device__ __forceinline__ void pw_fetch(const float* __restrict__ X, int64_t n, int D, int64_t row0, int k0, float (&r)[8]) {
    const int kk = threadIdx.x & 15, rr = threadIdx.x >> 4;
    const int k = k0 + kk;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int64_t row = row0 + rr + 16 * p;
        r[p] = (row < n && k < D) ? X[row * (int64_t)D + k] : 0.f;
    }
}
__device__ __forceinline__ void pw_stage(float* s, const float (&r)[8]) {
    const int kk = threadIdx.x & 15, rr = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < 8; ++p) s[kk * PW_LD + rr + 16 * p] = r[p];
}

// The fetch through an index table: src[p] is the row of X that the thread's tile row rr + 16 p reads (idx[row], the row itself
// without a table), -1 past the last row.  It is read once per tile; the fetch itself is pw_fetch with the row replaced.
__device__ __forceinline__ void pw_source_rows(const int* __restrict__ idx, int64_t n, int64_t row0, int (&src)[8]) {
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int64_t row = row0 + rr + 16 * p;
        src[p] = row < n ? (idx ? idx[row] : (int)row) : -1;
    }
}
__device__ __forceinline__ void pw_fetch_rows(const float* __restrict__ X, const int (&src)[8], int D, int k0, float (&r)[8]) {
    const int k = k0 + (threadIdx.x & 15);
#pragma unroll
    for (int p = 0; p < 8; ++p) r[p] = (src[p] >= 0 && k < D) ? X[src[p] * (int64_t)D + k] : 0.f;
}

// the two ways a tile operand is read: the rows row0 .. of X [n][D], or rows picked by an index table
struct PwRows {
    const float* __restrict__ X;
    int64_t n, row0;
    __device__ __forceinline__ void fetch(int D, int k0, float (&r)[8]) const { pw_fetch(X, n, D, row0, k0, r); }
};
struct PwGatheredRows {
    const float* __restrict__ X;
    int src[8];
    __device__ __forceinline__ void fetch(int D, int k0, float (&r)[8]) const { pw_fetch_rows(X, src, D, k0, r); }
};

// acc[i][j] = A[64 wm + 32 i ..][:] . B[64 wn + 32 j ..][:]^T for the wave (wm, wn) of the 2 x 2 waves
template <class RowsA, class RowsB>
__device__ __forceinline__ void pw_product_of(const RowsA& A, const RowsB& B, int D, PwShared& sh, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float ra[8], rb[8];
    A.fetch(D, 0, ra);
    B.fetch(D, 0, rb);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1, l31 = lane & 31, h = lane >> 5;
    for (int k0 = 0; k0 < D; k0 += PW_BK) {
        __syncthreads();
        pw_stage(sh.a, ra);
        pw_stage(sh.b, rb);
        __syncthreads();
        if (k0 + PW_BK < D) {
            A.fetch(D, k0 + PW_BK, ra);
            B.fetch(D, k0 + PW_BK, rb);
        }
#pragma unroll
        for (int kk = 0; kk < PW_BK; kk += 2) {
            const float* pa = sh.a + (kk + h) * PW_LD + wm * 64 + l31;
            const float* pb = sh.b + (kk + h) * PW_LD + wn * 64 + l31;
            const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// acc[i][j] = U[row0 + 64 wm + 32 i ..][:] . V[col0 + 64 wn + 32 j ..][:]^T
__device__ __forceinline__ void pw_product(const float* __restrict__ U, int64_t nu, int64_t row0, const float* __restrict__ V, int64_t nv,
                                           int64_t col0, int D, PwShared& sh, f32x16 (&acc)[2][2]) {
    pw_product_of(PwRows{U, nu, row0}, PwRows{V, nv, col0}, D, sh, acc);
}

// The waves of column half c write d(i, j) = max((norm_u[i] - 2 dot) + norm_v[j], 0) of their 64 x 64 quarter into sh.d
// [row][column of the half]; an element outside U or V is +inf: it wins no minimum and is under no radius.
__device__ __forceinline__ void pw_write_half(PwShared& sh, const f32x16 (&acc)[2][2], int c, int64_t row0, int64_t nu, int64_t col0, int64_t nv) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1, l31 = lane & 31, h = lane >> 5;
    if (wn != c) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, col = j * 32 + l31;
                float t = sh.nu[row] - 2.f * acc[i][j][r];
                t = t + sh.nv[c * 64 + col];
                float d = fmaxf(t, 0.f);
                if (row0 + row >= nu || col0 + c * 64 + col >= nv) d = INFINITY;
                sh.d[row * PW_DLD + col] = d;
            }
}

// the same staging of the dot products themselves (the padding is a product of zeros; the reader masks it by row and column)
__device__ __forceinline__ void pw_write_half_dots(PwShared& sh, const f32x16 (&acc)[2][2], int c) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1, l31 = lane & 31, h = lane >> 5;
    if (wn != c) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sh.d[(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * PW_DLD + j * 32 + l31] = acc[i][j][r];
}

template <int K> __device__ __forceinline__ void list_insert(float (&list)[K], float v) {
    if (v < list[K - 1]) {
        list[K - 1] = v;
#pragma unroll
        for (int q = K - 1; q > 0; --q) {
            const float lo = fminf(list[q - 1], list[q]), hi = fmaxf(list[q - 1], list[q]);
            list[q - 1] = lo;
            list[q] = hi;
        }
    }
}

__device__ __forceinline__ void pw_tile_range(int64_t tiles_n, int S, int s, int64_t& t0, int64_t& t1) {
    t0 = tiles_n * s / S;
    t1 = tiles_n * (s + 1) / S;
}

// parts[row][2 s + half][0 .. k1): the k1 smallest of the row's distances to the columns of split s that thread `half` of the
// row's pair scanned, ascending (+inf where it saw fewer than k1)
template <int K>
__global__ __launch_bounds__(256) void pw_ksmallest_kernel(const float* __restrict__ U, int64_t nu, const float* __restrict__ V, int64_t nv, int D,
                                                           const float* __restrict__ norm_u, const float* __restrict__ norm_v, int k1,
                                                           float* __restrict__ parts, int S, int64_t tiles_n) {
    __shared__ PwShared sh;
    const int t = threadIdx.x, s = (int)(blockIdx.x % S);
    const int64_t row0 = (int64_t)(blockIdx.x / S) * PW_T;
    if (t < PW_T) sh.nu[t] = row0 + t < nu ? norm_u[row0 + t] : 0.f;
    float list[K];
#pragma unroll
    for (int q = 0; q < K; ++q) list[q] = INFINITY;
    int64_t t0, t1;
    pw_tile_range(tiles_n, S, s, t0, t1);
    f32x16 acc[2][2];
    for (int64_t ct = t0; ct < t1; ++ct) {
        const int64_t col0 = ct * PW_T;
        __syncthreads();
        if (t < PW_T) sh.nv[t] = col0 + t < nv ? norm_v[col0 + t] : 0.f;
        pw_product(U, nu, row0, V, nv, col0, D, sh, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c) __syncthreads();
            pw_write_half(sh, acc, c, row0, nu, col0, nv);
            __syncthreads();
            const float* drow = sh.d + (t >> 1) * PW_DLD + (t & 1) * 32;
            for (int j = 0; j < 32; ++j) list_insert<K>(list, drow[j]);
        }
    }
    const int64_t row = row0 + (t >> 1);
    if (row < nu) {
        float* o = parts + (row * (2 * S) + 2 * s + (t & 1)) * (int64_t)k1;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < k1) o[q] = list[q];
    }
}

// out[row][0 .. k1) = the k1 smallest of the row's P lists of k1, ascending.  Selection moves values and rounds nothing, so
// the order in which the lists are taken does not show in the result; it is fixed all the same (p ascending).
__global__ __launch_bounds__(256) void ksmallest_merge_kernel(const float* __restrict__ parts, int64_t n, int P, int k1, int64_t part_stride,
                                                              int64_t row_stride, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    float list[PW_KMAX];
#pragma unroll
    for (int q = 0; q < PW_KMAX; ++q) list[q] = INFINITY;
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < k1; ++q) list_insert<PW_KMAX>(list, parts[row * row_stride + p * part_stride + q]);
#pragma unroll
    for (int q = 0; q < PW_KMAX; ++q)
        if (q < k1) out[row * k1 + q] = list[q];
}

// u_in[i][c] |= any_j d(i, j) <= radii_v[j][c];  v_in[j][c] |= any_i d(i, j) <= radii_u[i][c].  A flag byte only ever goes
// from 0 to 1, so the OR is a plain byte store of 1 by whoever finds a pair: every writer of a byte writes the same value.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_within_kernel(const float* __restrict__ U, int64_t nu, const float* __restrict__ V, int64_t nv, int D,
                                                        const float* __restrict__ norm_u, const float* __restrict__ norm_v,
                                                        const float* __restrict__ radii_u, int Ku, const float* __restrict__ radii_v, int Kv,
                                                        uint8_t* __restrict__ u_in, uint8_t* __restrict__ v_in, int S, int64_t tiles_n) {
    __shared__ PwShared sh;
    const int t = threadIdx.x, s = (int)(blockIdx.x % S);
    const int64_t row0 = (int64_t)(blockIdx.x / S) * PW_T;
    if (t < PW_T) {
        const bool in = row0 + t < nu;
        sh.nu[t] = in ? norm_u[row0 + t] : 0.f;
#pragma unroll
        for (int c = 0; c < PW_RMAX; ++c) sh.ru[t * PW_RMAX + c] = (in && c < Ku) ? radii_u[(row0 + t) * Ku + c] : -1.f;
    }
    int64_t t0, t1;
    pw_tile_range(tiles_n, S, s, t0, t1);
    f32x16 acc[2][2];
    unsigned uf = 0;
    for (int64_t ct = t0; ct < t1; ++ct) {
        const int64_t col0 = ct * PW_T;
        __syncthreads();
        if (t < PW_T) {
            const bool in = col0 + t < nv;
            sh.nv[t] = in ? norm_v[col0 + t] : 0.f;
#pragma unroll
            for (int c = 0; c < PW_RMAX; ++c) sh.rv[t * PW_RMAX + c] = (in && c < Kv) ? radii_v[(col0 + t) * Kv + c] : -1.f;
        }
        pw_product(U, nu, row0, V, nv, col0, D, sh, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c) __syncthreads();
            pw_write_half(sh, acc, c, row0, nu, col0, nv);
            __syncthreads();
            {   // this thread's row against the radii of 32 columns
                const float* drow = sh.d + (t >> 1) * PW_DLD + (t & 1) * 32;
                const float* rv = sh.rv + (c * 64 + (t & 1) * 32) * PW_RMAX;
#pragma unroll 4
                for (int j = 0; j < 32; ++j) {
                    const float d = drow[j];
#pragma unroll
                    for (int q = 0; q < PW_RMAX; ++q) uf |= (unsigned)(d <= rv[j * PW_RMAX + q]) << q;
                }
            }
            {   // this thread's column against the radii of 32 rows
                const int col = t & 63, r0 = (t >> 6) * 32;
                unsigned vf = 0;
#pragma unroll 4
                for (int r = r0; r < r0 + 32; ++r) {
                    const float d = sh.d[r * PW_DLD + col];
#pragma unroll
                    for (int q = 0; q < PW_RMAX; ++q) vf |= (unsigned)(d <= sh.ru[r * PW_RMAX + q]) << q;
                }
                const int64_t gc = col0 + c * 64 + col;
                if (gc < nv)
                    for (int q = 0; q < Ku; ++q)
                        if (vf >> q & 1) v_in[gc * Ku + q] = 1;
            }
        }
    }
    const int64_t row = row0 + (t >> 1);
    if (row < nu)
        for (int q = 0; q < Kv; ++q)
            if (uf >> q & 1) u_in[row * Kv + q] = 1;
}

// parts[b][row][2 s + half] = sum over the columns j of split s that thread `half` of the row's pair scanned, in ascending j, of
// (gamma (u_i . v_j) + coef0)^degree in float64: the f32 dot product widened, t = gamma dot + coef0, then t t .. t multiplied left
// to right.  Rows and columns of batch b are read through u_idx[b] / v_idx[b] (null: the rows themselves).  A column past nv adds
// nothing, and with skip neither does one whose source row is the row's own.  The column ids of a tile lie in sh.rv as integers.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_polysum_kernel(const float* __restrict__ U, int64_t nu, const float* __restrict__ V, int64_t nv, int D,
                                                         const int* __restrict__ u_idx, const int* __restrict__ v_idx, double gamma, double coef0,
                                                         int degree, int skip, double* __restrict__ parts, int S, int64_t tiles_n, int64_t tiles_m) {
    __shared__ PwShared sh;
    int* cid = reinterpret_cast<int*>(sh.rv);
    const int t = threadIdx.x, s = (int)(blockIdx.x % S);
    const int64_t rt = blockIdx.x / S, b = rt / tiles_m, row0 = rt % tiles_m * PW_T;
    const int* ui = u_idx ? u_idx + b * nu : nullptr;
    const int* vi = v_idx ? v_idx + b * nv : nullptr;
    PwGatheredRows ra{U, {}}, rb{V, {}};
    pw_source_rows(ui, nu, row0, ra.src);
    const int64_t row = row0 + (t >> 1);
    const int rid = (skip && row < nu) ? (ui ? ui[row] : (int)row) : -2;      // -2: no column has it, the diagonal stays
    int64_t t0, t1;
    pw_tile_range(tiles_n, S, s, t0, t1);
    f32x16 acc[2][2];
    double sum = 0.0;
    for (int64_t ct = t0; ct < t1; ++ct) {
        const int64_t col0 = ct * PW_T;
        __syncthreads();
        if (t < PW_T) cid[t] = col0 + t < nv ? (vi ? vi[col0 + t] : (int)(col0 + t)) : -1;
        pw_source_rows(vi, nv, col0, rb.src);
        pw_product_of(ra, rb, D, sh, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c) __syncthreads();
            pw_write_half_dots(sh, acc, c);
            __syncthreads();
            const float* drow = sh.d + (t >> 1) * PW_DLD + (t & 1) * 32;
            const int* ids = cid + c * 64 + (t & 1) * 32;
            for (int j = 0; j < 32; ++j) {
                const double x = gamma * (double)drow[j] + coef0;
                double p = x;
                for (int q = 1; q < degree; ++q) p = p * x;
                if (ids[j] >= 0 && ids[j] != rid) sum = sum + p;
            }
        }
    }
    if (row < nu) parts[(b * nu + row) * (2 * S) + 2 * s + (t & 1)] = sum;
}

// out[r] = parts[r][0] + parts[r][1] + ... + parts[r][P - 1], left to right
__global__ __launch_bounds__(256) void polysum_fold_kernel(const double* __restrict__ parts, int64_t n, int P, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double a = 0.0;
    for (int p = 0; p < P; ++p) a = a + parts[r * P + p];
    out[r] = a;
}

// One pass over d(i, j) against the radii of the columns, strictly below (pw_within_kernel takes <=):
//   parts[row][2 s + half][q] = #{ j scanned by thread `half` of the row's pair in split s : d(row, j) < radii_v[j][q] }
//   v_in[j][q] = 1 if any row i has d(i, j) < radii_v[j][q], the byte store of pw_within_kernel
// Counts are integers: no order or chunking shows in them.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_count_within_kernel(const float* __restrict__ U, int64_t nu, const float* __restrict__ V, int64_t nv, int D,
                                                              const float* __restrict__ norm_u, const float* __restrict__ norm_v,
                                                              const float* __restrict__ radii_v, int Kv, int* __restrict__ parts,
                                                              uint8_t* __restrict__ v_in, int S, int64_t tiles_n) {
    __shared__ PwShared sh;
    const int t = threadIdx.x, s = (int)(blockIdx.x % S);
    const int64_t row0 = (int64_t)(blockIdx.x / S) * PW_T;
    if (t < PW_T) sh.nu[t] = row0 + t < nu ? norm_u[row0 + t] : 0.f;
    int64_t t0, t1;
    pw_tile_range(tiles_n, S, s, t0, t1);
    f32x16 acc[2][2];
    int cnt[PW_RMAX] = {0, 0, 0, 0};
    for (int64_t ct = t0; ct < t1; ++ct) {
        const int64_t col0 = ct * PW_T;
        __syncthreads();
        if (t < PW_T) {
            const bool in = col0 + t < nv;
            sh.nv[t] = in ? norm_v[col0 + t] : 0.f;
#pragma unroll
            for (int c = 0; c < PW_RMAX; ++c) sh.rv[t * PW_RMAX + c] = (in && c < Kv) ? radii_v[(col0 + t) * Kv + c] : -1.f;
        }
        pw_product(U, nu, row0, V, nv, col0, D, sh, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c) __syncthreads();
            pw_write_half(sh, acc, c, row0, nu, col0, nv);
            __syncthreads();
            {   // this thread's row against the radii of 32 columns
                const float* drow = sh.d + (t >> 1) * PW_DLD + (t & 1) * 32;
                const float* rv = sh.rv + (c * 64 + (t & 1) * 32) * PW_RMAX;
#pragma unroll 4
                for (int j = 0; j < 32; ++j) {
                    const float d = drow[j];
#pragma unroll
                    for (int q = 0; q < PW_RMAX; ++q) cnt[q] += (int)(d < rv[j * PW_RMAX + q]);
                }
            }
            {   // this thread's column, with its own radii, against 32 rows
                const int col = t & 63, r0 = (t >> 6) * 32;
                float rq[PW_RMAX];
#pragma unroll
                for (int q = 0; q < PW_RMAX; ++q) rq[q] = sh.rv[(c * 64 + col) * PW_RMAX + q];
                unsigned vf = 0;
#pragma unroll 4
                for (int r = r0; r < r0 + 32; ++r) {
                    const float d = sh.d[r * PW_DLD + col];
#pragma unroll
                    for (int q = 0; q < PW_RMAX; ++q) vf |= (unsigned)(d < rq[q]) << q;
                }
                const int64_t gc = col0 + c * 64 + col;
                if (gc < nv)
                    for (int q = 0; q < Kv; ++q)
                        if (vf >> q & 1) v_in[gc * Kv + q] = 1;
            }
        }
    }
    const int64_t row = row0 + (t >> 1);
    if (row < nu) {
        int* o = parts + (row * (2 * S) + 2 * s + (t & 1)) * (int64_t)Kv;
#pragma unroll
        for (int q = 0; q < PW_RMAX; ++q)
            if (q < Kv) o[q] = cnt[q];
    }
}

// u_count[row][q] += parts[row][0][q] + ... + parts[row][P - 1][q]: thread e owns element e = row * Kv + q
__global__ __launch_bounds__(256) void count_fold_kernel(const int* __restrict__ parts, int64_t n, int P, int Kv, int* __restrict__ u_count) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * Kv) return;
    const int64_t row = e / Kv;
    const int q = (int)(e % Kv);
    int a = 0;
    for (int p = 0; p < P; ++p) a += parts[(row * P + p) * Kv + q];
    u_count[e] += a;
}

// out[i] = sum_k X[i][k]^2: one wave per row, lane l adds k = l, l + 64, ... ascending into one accumulator, then the 64
// partial sums fold by the xor butterfly 32, 16, .. 1
__global__ __launch_bounds__(256) void row_sqnorms_kernel(const float* __restrict__ X, int64_t n, int D, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* x = X + row * (int64_t)D;
    float s = 0.f;
    for (int k = threadIdx.x & 63; k < D; k += 64) s = s + x[k] * x[k];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) out[row] = s;
}

// mu[c] = (sum_i (double)X[i][c]) / n: thread (c, p) of 16 x 16 adds the rows p, p + 16, ... ascending, the 16 partial sums of
// a column are added p = 0 .. 15 ascending
__global__ __launch_bounds__(256) void col_mean_f64_kernel(const float* __restrict__ X, int64_t n, int D, double* __restrict__ mu) {
    __shared__ double part[16][17];
    const int c = threadIdx.x & 15, p = threadIdx.x >> 4;
    const int64_t col = (int64_t)blockIdx.x * 16 + c;
    double s = 0.0;
    if (col < D)
        for (int64_t i = p; i < n; i += 16) s = s + (double)X[i * D + col];
    part[p][c] = s;
    __syncthreads();
    if (p == 0 && col < D) {
        double a = 0.0;
        for (int q = 0; q < 16; ++q) a = a + part[q][c];
        mu[col] = a / (double)n;
    }
}

constexpr int CV_T = 64, CV_KC = 16;

__device__ __forceinline__ void cv_fetch(const float* __restrict__ X, int64_t n, int D, int64_t i0, int64_t col, double m, double (&r)[4]) {
    const int rr = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = i0 + rr + 4 * p;
        r[p] = (i < n && col < D) ? (double)X[i * D + col] - m : 0.0;
    }
}

// sigma = (X - mu)^T (X - mu) / (n - 1) in f64 on the vector unit: one block per 64 x 64 tile of the upper triangle, a 4 x 4
// micro-tile per thread, every element one fma chain over the rows i = 0 .. n-1 ascending (the padding past n appends
// fma(0, 0, acc)).  The centred values are formed once, (double)x - mu, so both factors of a product are the same numbers
// whichever of (a, b) and (b, a) is computed; only a <= b is computed and the value is stored at both places.
__global__ __launch_bounds__(256) void cov_f64_kernel(const float* __restrict__ X, int64_t n, int D, const double* __restrict__ mu,
                                                      double* __restrict__ sigma, int tiles) {
    __shared__ double As[CV_KC * CV_T], Bs[CV_KC * CV_T];
    int ti = 0, rem = (int)blockIdx.x;
    while (rem >= tiles - ti) {
        rem -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lc = t & 63, lr = t >> 6;
    const int64_t ca = (int64_t)ti * CV_T + lc, cb = (int64_t)tj * CV_T + lc;
    const double ma = ca < D ? mu[ca] : 0.0, mb = cb < D ? mu[cb] : 0.0;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    double ra[4], rb[4];
    cv_fetch(X, n, D, 0, ca, ma, ra);
    cv_fetch(X, n, D, 0, cb, mb, rb);
    for (int64_t i0 = 0; i0 < n; i0 += CV_KC) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            As[(lr + 4 * p) * CV_T + lc] = ra[p];
            Bs[(lr + 4 * p) * CV_T + lc] = rb[p];
        }
        __syncthreads();
        if (i0 + CV_KC < n) {
            cv_fetch(X, n, D, i0 + CV_KC, ca, ma, ra);
            cv_fetch(X, n, D, i0 + CV_KC, cb, mb, rb);
        }
#pragma unroll
        for (int k = 0; k < CV_KC; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[k * CV_T + ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[k * CV_T + tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
    }
    const double den = (double)(n - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t a = (int64_t)ti * CV_T + ty * 4 + i, b = (int64_t)tj * CV_T + tx + 16 * j;
            if (a < D && b < D && a <= b) {
                const double v = acc[i][j] / den;
                sigma[a * D + b] = v;
                sigma[b * D + a] = v;
            }
        }
}

// logits[i][c] = sum_k X[i][k] Wt[c][k]: block b owns row tile b / tiles_c and column tile b % tiles_c (the 8 column tiles of the
// real head land on the 8 XCDs, each of which keeps its 1 MB slice of Wt in L2).  Rows >= n and columns >= C are products of the
// zero padding and are not stored.
__global__ __launch_bounds__(256) void head_logits_kernel(const float* __restrict__ X, int64_t n, int D, const float* __restrict__ Wt, int C,
                                                          float* __restrict__ logits, int64_t ld, int tiles_c) {
    __shared__ PwShared sh;
    const int64_t row0 = (int64_t)(blockIdx.x / tiles_c) * PW_T, col0 = (int64_t)(blockIdx.x % tiles_c) * PW_T;
    f32x16 acc[2][2];
    pw_product(X, n, row0, Wt, C, col0, D, sh, acc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = row0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, col = col0 + wn * 64 + j * 32 + l31;
                if (row < n && col < C) logits[row * ld + col] = acc[i][j][r];
            }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// One wave per row, every sum 64 lane-strided partials in ascending c folded by the xor butterfly.  From logits: m = max_c l_c,
// lse = m + log sum_c exp(l_c - m), h = sum_c p_c (l_c - lse) with p_c = exp(l_c - lse).  PROBS: the row holds p_c itself,
// h = sum_c p_c log p_c and lse is written as 0.  A term with p = 0 is its limit 0.
template <bool PROBS>
__global__ __launch_bounds__(256) void is_rows_kernel(const float* __restrict__ in, int64_t n, int C, int64_t ld, double* __restrict__ lse,
                                                      double* __restrict__ h) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* x = in + row * ld;
    const int lane = threadIdx.x & 63;
    double L = 0.0, hs = 0.0;
    if constexpr (!PROBS) {
        float mf = -INFINITY;
        for (int c = lane; c < C; c += 64) mf = fmaxf(mf, x[c]);
        const double m = (double)wave_max(mf);
        double s = 0.0;
        for (int c = lane; c < C; c += 64) s = s + exp((double)x[c] - m);
        L = m + log(wave_sum_f64(s));
    }
    for (int c = lane; c < C; c += 64) {
        const double g = PROBS ? 0.0 : (double)x[c] - L;
        const double p = PROBS ? (double)x[c] : exp(g);
        if (p > 0.0) hs = hs + p * (PROBS ? log(p) : g);
    }
    hs = wave_sum_f64(hs);
    if (lane == 0) {
        lse[row] = L;
        h[row] = hs;
    }
}

// colsum[s][c] = sum of p_ic over the rows i of split s, one chain in ascending i per (s, c): thread (k, c) walks the rows of
// the launch (global rows row0 .. row0 + n) that lie in split s = row0 / split + k.  A split that began in an earlier launch is
// continued from the value in memory, which a float64 store and load return unchanged: the chain does not see the cut.
template <bool PROBS>
__global__ __launch_bounds__(64) void is_colsums_kernel(const float* __restrict__ in, const double* __restrict__ lse, int64_t n, int C, int64_t ld,
                                                        int64_t row0, int64_t split, double* __restrict__ colsum) {
    const int c = (int)blockIdx.y * 64 + threadIdx.x;
    if (c >= C) return;
    const int64_t s = row0 / split + blockIdx.x;
    const int64_t a = s * split > row0 ? s * split : row0, b = (s + 1) * split < row0 + n ? (s + 1) * split : row0 + n;
    double* out = colsum + s * C + c;
    double acc = a == s * split ? 0.0 : *out;
#pragma unroll 4
    for (int64_t g = a; g < b; ++g) {
        const int64_t i = g - row0;
        const double v = (double)in[i * ld + c];
        acc = acc + (PROBS ? v : exp(v - lse[i]));
    }
    *out = acc;
}

// scores[s] = exp(H - sum_c m_c log m_c), H = (sum_i h_i) / n_s over the rows of split s, m_c = colsum[s][c] / n_s: one wave per
// split, both sums lane-strided partials in ascending index and the xor butterfly; m_c = 0 adds its limit 0.
__global__ __launch_bounds__(64) void is_finish_kernel(const double* __restrict__ h, const double* __restrict__ colsum, int64_t N, int C, int64_t split,
                                                       double* __restrict__ scores) {
    const int64_t s = blockIdx.x, a = s * split, b = a + split < N ? a + split : N;
    const int lane = threadIdx.x;
    const double ns = (double)(b - a);
    double hs = 0.0, e = 0.0;
    for (int64_t i = a + lane; i < b; i += 64) hs = hs + h[i];
    for (int c = lane; c < C; c += 64) {
        const double m = colsum[s * C + c] / ns;
        if (m > 0.0) e = e + m * log(m);
    }
    hs = wave_sum_f64(hs);
    e = wave_sum_f64(e);
    if (lane == 0) scores[s] = exp(hs / ns - e);
}

int pw_splits(int64_t nv) {
    const int64_t tiles = (nv + PW_T - 1) / PW_T;
    return (int)(tiles < PW_SPLITS ? tiles : PW_SPLITS);
}

bool pw_sizes_ok(const char* name, int64_t nu, int64_t nv, int D) {
    // one block per (row tile, split) in a 1-D grid
    if (nu < 1 || nv < 1 || D < 1 || nu > ((int64_t)1 << 31) - PW_T || nv > ((int64_t)1 << 31) - PW_T ||
        (nu + PW_T - 1) / PW_T * PW_SPLITS > 0x7fffffff) {
        vaw_set_error("%s: sizes nu %lld nv %lld D %d out of range", name, (long long)nu, (long long)nv, D);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int vaw_row_sqnorms(const float* X, int64_t n, int D, float* out, vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && D >= 1 && (n + 3) / 4 <= 0x7fffffff, "vaw_row_sqnorms: sizes n %lld D %d out of range", (long long)n, D);
    VAW_CHECK_ARG(X && out, "vaw_row_sqnorms: null pointer");
    row_sqnorms_kernel<<<dim3((unsigned)((n + 3) / 4)), 256, 0, (hipStream_t)stream>>>(X, n, D, out);
    VAW_CHECK_LAUNCH("vaw_row_sqnorms");
    return VAW_OK;
}

int64_t vaw_pairwise_workspace_bytes(int64_t nu, int64_t nv, int k1) {
    if (nu < 1 || nv < 1 || k1 < 1 || k1 > PW_KMAX) return 0;
    return nu * 2 * pw_splits(nv) * k1 * (int64_t)sizeof(float);
}

int vaw_ksmallest_merge(const float* parts, int64_t n, int P, int k1, int64_t part_stride, int64_t row_stride, float* out,
                        vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && P >= 1 && k1 >= 1 && k1 <= PW_KMAX && part_stride >= 1 && row_stride >= 1 && (n + 255) / 256 <= 0x7fffffff,
                  "vaw_ksmallest_merge: sizes n %lld P %d k1 %d strides %lld %lld out of range (k1 in 1 .. %d)", (long long)n, P, k1,
                  (long long)part_stride, (long long)row_stride, PW_KMAX);
    VAW_CHECK_ARG(parts && out, "vaw_ksmallest_merge: null pointer");
    ksmallest_merge_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(parts, n, P, k1, part_stride, row_stride, out);
    VAW_CHECK_LAUNCH("vaw_ksmallest_merge");
    return VAW_OK;
}

int vaw_pairwise_ksmallest(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                           int k1, float* out, void* ws, int64_t ws_bytes, vaw_stream stream) {
    if (!pw_sizes_ok("vaw_pairwise_ksmallest", nu, nv, D)) return VAW_ERR_INVALID;
    VAW_CHECK_ARG(k1 >= 1 && k1 <= PW_KMAX && k1 <= nv, "vaw_pairwise_ksmallest: k1 %d outside 1 .. min(%d, nv = %lld)", k1, PW_KMAX,
                  (long long)nv);
    VAW_CHECK_ARG(U && V && norm_u && norm_v && out && ws, "vaw_pairwise_ksmallest: null pointer");
    const int64_t need = vaw_pairwise_workspace_bytes(nu, nv, k1);
    VAW_CHECK_ARG(ws_bytes >= need, "vaw_pairwise_ksmallest: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    const int S = pw_splits(nv);
    const int64_t tiles_m = (nu + PW_T - 1) / PW_T, tiles_n = (nv + PW_T - 1) / PW_T;
    const dim3 grid((unsigned)(tiles_m * S));
    float* parts = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    if (k1 <= 4) pw_ksmallest_kernel<4><<<grid, 256, 0, st>>>(U, nu, V, nv, D, norm_u, norm_v, k1, parts, S, tiles_n);
    else if (k1 <= 8) pw_ksmallest_kernel<8><<<grid, 256, 0, st>>>(U, nu, V, nv, D, norm_u, norm_v, k1, parts, S, tiles_n);
    else pw_ksmallest_kernel<16><<<grid, 256, 0, st>>>(U, nu, V, nv, D, norm_u, norm_v, k1, parts, S, tiles_n);
    VAW_CHECK_LAUNCH("vaw_pairwise_ksmallest");
    return vaw_ksmallest_merge(parts, nu, 2 * S, k1, k1, (int64_t)2 * S * k1, out, stream);
}

int vaw_pairwise_within(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                        const float* radii_u, int Ku, const float* radii_v, int Kv, uint8_t* u_in, uint8_t* v_in, vaw_stream stream) {
    if (!pw_sizes_ok("vaw_pairwise_within", nu, nv, D)) return VAW_ERR_INVALID;
    VAW_CHECK_ARG(Ku >= 1 && Ku <= PW_RMAX && Kv >= 1 && Kv <= PW_RMAX, "vaw_pairwise_within: Ku %d Kv %d outside 1 .. %d", Ku, Kv, PW_RMAX);
    VAW_CHECK_ARG(U && V && norm_u && norm_v && radii_u && radii_v && u_in && v_in, "vaw_pairwise_within: null pointer");
    const int S = pw_splits(nv);
    const int64_t tiles_m = (nu + PW_T - 1) / PW_T, tiles_n = (nv + PW_T - 1) / PW_T;
    pw_within_kernel<<<dim3((unsigned)(tiles_m * S)), 256, 0, (hipStream_t)stream>>>(U, nu, V, nv, D, norm_u, norm_v, radii_u, Ku, radii_v, Kv,
                                                                                    u_in, v_in, S, tiles_n);
    VAW_CHECK_LAUNCH("vaw_pairwise_within");
    return VAW_OK;
}

int64_t vaw_pairwise_polysum_workspace_bytes(int64_t nu, int64_t nv, int batches) {
    if (nu < 1 || nv < 1 || batches < 1) return 0;
    return (int64_t)batches * nu * 2 * pw_splits(nv) * (int64_t)sizeof(double);
}

int vaw_pairwise_polysum(const float* U, int64_t nu, const float* V, int64_t nv, int D, const int32_t* u_idx, const int32_t* v_idx, int batches,
                         double gamma, double coef0, int degree, int skip_diagonal, double* rowsum, void* ws, int64_t ws_bytes,
                         vaw_stream stream) {
    if (!pw_sizes_ok("vaw_pairwise_polysum", nu, nv, D)) return VAW_ERR_INVALID;
    const int S = pw_splits(nv);
    const int64_t tiles_m = (nu + PW_T - 1) / PW_T, tiles_n = (nv + PW_T - 1) / PW_T;
    VAW_CHECK_ARG(batches >= 1 && (int64_t)batches * tiles_m * S <= 0x7fffffff && ((int64_t)batches * nu + 255) / 256 <= 0x7fffffff,
                  "vaw_pairwise_polysum: batches %d out of range for nu %lld nv %lld", batches, (long long)nu, (long long)nv);
    VAW_CHECK_ARG(degree >= 1 && degree <= 8, "vaw_pairwise_polysum: degree %d outside 1 .. 8", degree);
    VAW_CHECK_ARG(isfinite(gamma) && isfinite(coef0), "vaw_pairwise_polysum: gamma %g or coef0 %g is not finite", gamma, coef0);
    VAW_CHECK_ARG(U && V && rowsum && ws, "vaw_pairwise_polysum: null pointer");
    const int64_t need = vaw_pairwise_polysum_workspace_bytes(nu, nv, batches);
    VAW_CHECK_ARG(ws_bytes >= need, "vaw_pairwise_polysum: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    double* parts = (double*)ws;
    hipStream_t st = (hipStream_t)stream;
    pw_polysum_kernel<<<dim3((unsigned)(batches * tiles_m * S)), 256, 0, st>>>(U, nu, V, nv, D, u_idx, v_idx, gamma, coef0, degree,
                                                                             skip_diagonal != 0, parts, S, tiles_n, tiles_m);
    VAW_CHECK_LAUNCH("vaw_pairwise_polysum");
    const int64_t rows = (int64_t)batches * nu;
    polysum_fold_kernel<<<dim3((unsigned)((rows + 255) / 256)), 256, 0, st>>>(parts, rows, 2 * S, rowsum);
    VAW_CHECK_LAUNCH("vaw_pairwise_polysum");
    return VAW_OK;
}

int64_t vaw_pairwise_count_workspace_bytes(int64_t nu, int64_t nv, int Kv) {
    if (nu < 1 || nv < 1 || Kv < 1 || Kv > PW_RMAX) return 0;
    return nu * 2 * pw_splits(nv) * Kv * (int64_t)sizeof(int32_t);
}

int vaw_pairwise_count_within(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                              const float* radii_v, int Kv, int32_t* u_count, uint8_t* v_in, void* ws, int64_t ws_bytes, vaw_stream stream) {
    if (!pw_sizes_ok("vaw_pairwise_count_within", nu, nv, D)) return VAW_ERR_INVALID;
    VAW_CHECK_ARG(Kv >= 1 && Kv <= PW_RMAX, "vaw_pairwise_count_within: Kv %d outside 1 .. %d", Kv, PW_RMAX);
    VAW_CHECK_ARG(U && V && norm_u && norm_v && radii_v && u_count && v_in && ws, "vaw_pairwise_count_within: null pointer");
    const int64_t need = vaw_pairwise_count_workspace_bytes(nu, nv, Kv);
    VAW_CHECK_ARG(ws_bytes >= need, "vaw_pairwise_count_within: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    const int S = pw_splits(nv);
    const int64_t tiles_m = (nu + PW_T - 1) / PW_T, tiles_n = (nv + PW_T - 1) / PW_T;
    int* parts = (int*)ws;
    hipStream_t st = (hipStream_t)stream;
    pw_count_within_kernel<<<dim3((unsigned)(tiles_m * S)), 256, 0, st>>>(U, nu, V, nv, D, norm_u, norm_v, radii_v, Kv, parts, v_in, S, tiles_n);
    VAW_CHECK_LAUNCH("vaw_pairwise_count_within");
    count_fold_kernel<<<dim3((unsigned)((nu * Kv + 255) / 256)), 256, 0, st>>>(parts, nu, 2 * S, Kv, u_count);
    VAW_CHECK_LAUNCH("vaw_pairwise_count_within");
    return VAW_OK;
}

int vaw_col_mean_f64(const float* X, int64_t n, int D, double* mu, vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && D >= 1, "vaw_col_mean_f64: sizes n %lld D %d out of range", (long long)n, D);
    VAW_CHECK_ARG(X && mu, "vaw_col_mean_f64: null pointer");
    col_mean_f64_kernel<<<dim3((unsigned)((D + 15) / 16)), 256, 0, (hipStream_t)stream>>>(X, n, D, mu);
    VAW_CHECK_LAUNCH("vaw_col_mean_f64");
    return VAW_OK;
}

int vaw_cov_f64(const float* X, int64_t n, int D, const double* mu, double* sigma, vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && D >= 1 && D <= 1 << 20, "vaw_cov_f64: sizes n %lld D %d out of range", (long long)n, D);
    VAW_CHECK_ARG(X && mu && sigma, "vaw_cov_f64: null pointer");
    const int tiles = (D + CV_T - 1) / CV_T;
    const int64_t blocks = (int64_t)tiles * (tiles + 1) / 2;
    cov_f64_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(X, n, D, mu, sigma, tiles);
    VAW_CHECK_LAUNCH("vaw_cov_f64");
    return VAW_OK;
}

int vaw_head_logits(const float* X, int64_t n, int D, const float* Wt, int C, float* logits, int64_t ld, vaw_stream stream) {
    const int64_t tiles_m = (n + PW_T - 1) / PW_T, tiles_c = ((int64_t)C + PW_T - 1) / PW_T;
    VAW_CHECK_ARG(n >= 1 && D >= 1 && C >= 1 && ld >= C && n <= ((int64_t)1 << 31) - PW_T && C <= (1 << 30) && tiles_m * tiles_c <= 0x7fffffff,
                  "vaw_head_logits: sizes n %lld D %d C %d ld %lld out of range", (long long)n, D, C, (long long)ld);
    VAW_CHECK_ARG(X && Wt && logits, "vaw_head_logits: null pointer");
    head_logits_kernel<<<dim3((unsigned)(tiles_m * tiles_c)), 256, 0, (hipStream_t)stream>>>(X, n, D, Wt, C, logits, ld, (int)tiles_c);
    VAW_CHECK_LAUNCH("vaw_head_logits");
    return VAW_OK;
}

int vaw_is_rows(const float* in, int64_t n, int C, int64_t ld, int probs, double* lse, double* h, vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && C >= 1 && ld >= C && (n + 3) / 4 <= 0x7fffffff, "vaw_is_rows: sizes n %lld C %d ld %lld out of range", (long long)n, C,
                  (long long)ld);
    VAW_CHECK_ARG(in && lse && h, "vaw_is_rows: null pointer");
    const dim3 grid((unsigned)((n + 3) / 4));
    if (probs) is_rows_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(in, n, C, ld, lse, h);
    else is_rows_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(in, n, C, ld, lse, h);
    VAW_CHECK_LAUNCH("vaw_is_rows");
    return VAW_OK;
}

int vaw_is_colsums(const float* in, const double* lse, int64_t n, int C, int64_t ld, int probs, int64_t row0, int64_t split_size, double* colsum,
                   vaw_stream stream) {
    VAW_CHECK_ARG(n >= 1 && C >= 1 && ld >= C && row0 >= 0 && row0 <= ((int64_t)1 << 40) && n <= ((int64_t)1 << 40) && split_size >= 1 &&
                      split_size <= ((int64_t)1 << 40) && C <= 65535 * 64,
                  "vaw_is_colsums: sizes n %lld C %d ld %lld row0 %lld split_size %lld out of range", (long long)n, C, (long long)ld, (long long)row0,
                  (long long)split_size);
    const int64_t splits = (row0 + n - 1) / split_size - row0 / split_size + 1;
    VAW_CHECK_ARG(splits <= 0x7fffffff, "vaw_is_colsums: %lld splits in one launch", (long long)splits);
    VAW_CHECK_ARG(in && colsum && (probs || lse), "vaw_is_colsums: null pointer");
    const dim3 grid((unsigned)splits, (unsigned)((C + 63) / 64));
    if (probs) is_colsums_kernel<true><<<grid, 64, 0, (hipStream_t)stream>>>(in, lse, n, C, ld, row0, split_size, colsum);
    else is_colsums_kernel<false><<<grid, 64, 0, (hipStream_t)stream>>>(in, lse, n, C, ld, row0, split_size, colsum);
    VAW_CHECK_LAUNCH("vaw_is_colsums");
    return VAW_OK;
}

int vaw_is_finish(const double* h, const double* colsum, int64_t N, int C, int64_t split_size, double* scores, vaw_stream stream) {
    VAW_CHECK_ARG(N >= 1 && N <= ((int64_t)1 << 40) && C >= 1 && split_size >= 1 && split_size <= ((int64_t)1 << 40) && (N + split_size - 1) / split_size <= 0x7fffffff,
                  "vaw_is_finish: sizes N %lld C %d split_size %lld out of range", (long long)N, C, (long long)split_size);
    VAW_CHECK_ARG(h && colsum && scores, "vaw_is_finish: null pointer");
    is_finish_kernel<<<dim3((unsigned)((N + split_size - 1) / split_size)), 64, 0, (hipStream_t)stream>>>(h, colsum, N, C, split_size, scores);
    VAW_CHECK_LAUNCH("vaw_is_finish");
    return VAW_OK;
}

}  // extern "C"

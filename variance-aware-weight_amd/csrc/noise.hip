// Per-sample seeded noise: out[b, :] is a pure function of (seeds[b], draw, tag, element index) and of nothing else -- not of
// B, of the grid, of the stream or of what was drawn before.  Counter-based: block c of row b (elements 4c .. 4c+3) is
// Philox4x32-10 (Salmon et al., SC'11; the Random123 definition) under the key (low, high 32 bits of seeds[b] as an unsigned
// 64-bit pattern) at the counter (c, draw, tag, 0).  One lane computes one block and stores it once; the last block of a row
// whose length is no multiple of 4, and every block of a row that does not start on a vector boundary, are stored element
// by element.  Plain C++: no atomics, no device-side counter, no state.
#include "common.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;          // the key of the next round (unused after the tenth)
        k1 += PHILOX_W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// (0, 1]: the word rounded to float32, then ONE fused multiply-add (2^-32 r + 2^-33 is exact before its rounding)
__device__ __forceinline__ float philox_uniform(uint32_t r) { return fmaf((float)r, 0x1p-32f, 0x1p-33f); }

// Box-Muller on a pair of words: sqrt(-2 log u0) * (cos, sin)(2 pi u1); sincospif takes the angle in half turns, so 2 u1 is exact
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
    const float rad = sqrtf(-2.f * logf(philox_uniform(ra)));
    float s, c;
    sincospif(2.f * philox_uniform(rb), &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// the four values of a block in the output type
template <int MODE> __device__ __forceinline__ void noise_values(const uint32_t (&r)[4], uint32_t* v) {
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
}
template <int MODE, typename T> __device__ __forceinline__ void noise_values(const uint32_t (&r)[4], T* v) {
    float f[4];
    if constexpr (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = philox_uniform(r[j]);
    } else {
        box_muller(r[0], r[1], f[0], f[1]);
        box_muller(r[2], r[3], f[2], f[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (T)f[j];          // bf16: round to nearest even; double: exact
}

// one block in one go: 16 bytes (float, raw words), 8 bytes (bf16), two 16-byte halves (double)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_block(uint32_t* p, const uint32_t* v) {
    const u32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<u32x4*>(p) = t;
}
__device__ __forceinline__ void store_block(float* p, const float* v) { storew<4>(p, v); }
__device__ __forceinline__ void store_block(double* p, const double* v) { storew<4>(p, v); }
__device__ __forceinline__ void store_block(bf16_t* p, const bf16_t* v) {
    const bf16x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<bf16x4*>(p) = t;
}
template <typename T> constexpr uintptr_t block_align() { return sizeof(T) == 2 ? 8 : 16; }

template <int MODE, typename T>
__global__ void randn_seeded_kernel(T* __restrict__ out, const int64_t* __restrict__ seeds, int B, int64_t per_sample, uint32_t draw,
                                    uint32_t tag) {
    const int64_t blocks = (per_sample + 3) >> 2;          // <= 2^32: per_sample < 2^34
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint64_t seed = (uint64_t)seeds[b];
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        T* row = out + (int64_t)b * per_sample;
        const bool aligned = ((uintptr_t)row & (block_align<T>() - 1)) == 0;
        for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < blocks; c += (int64_t)gridDim.x * blockDim.x) {
            uint32_t r[4];
            philox4x32_10((uint32_t)c, draw, tag, 0u, k0, k1, r);
            T v[4];
            noise_values<MODE>(r, v);
            const int64_t e = 4 * c;
            if (aligned && e + 4 <= per_sample) {
                store_block(row + e, v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < per_sample) row[e + j] = v[j];
            }
        }
    }
}

template <int MODE, typename T>
static void launch_randn_seeded(void* out, const int64_t* seeds, int B, int64_t per_sample, int64_t draw, int tag, vaw_stream stream) {
    const int64_t g = (((per_sample + 3) >> 2) + 255) / 256;
    const dim3 grid((unsigned)(g > 1024 ? 1024 : g), (unsigned)(B > 65535 ? 65535 : B));          // grid-stride beyond, both ways
    randn_seeded_kernel<MODE, T><<<grid, 256, 0, (hipStream_t)stream>>>((T*)out, seeds, B, per_sample, (uint32_t)draw, (uint32_t)tag);
}

extern "C" int vaw_randn_seeded(void* out, int dtype, const int64_t* seeds, int B, int64_t per_sample, int64_t draw, int tag, int mode,
                                vaw_stream stream) {
    VAW_CHECK_ARG(out && seeds, "randn_seeded: null pointer");
    VAW_CHECK_ARG(B >= 1 && per_sample >= 1, "randn_seeded: bad sizes B=%d per_sample=%ld", B, (long)per_sample);
    VAW_CHECK_ARG(per_sample < ((int64_t)1 << 34), "randn_seeded: per_sample %ld >= 2^34 (the block counter is 32 bits)", (long)per_sample);
    VAW_CHECK_ARG(draw >= 0 && draw < ((int64_t)1 << 32), "randn_seeded: draw %ld outside [0, 2^32)", (long)draw);
    VAW_CHECK_ARG(tag >= 0, "randn_seeded: tag %d is negative", tag);
    VAW_CHECK_ARG(mode >= VAW_NOISE_BITS && mode <= VAW_NOISE_NORMAL, "randn_seeded: unknown mode %d", mode);
    VAW_CHECK_ARG(dtype == VAW_F32 || dtype == VAW_BF16 || dtype == VAW_F64, "randn_seeded: unknown dtype %d", dtype);
    VAW_CHECK_ARG(mode == VAW_NOISE_NORMAL || dtype == VAW_F32,
                  "randn_seeded: mode %d (raw words / uniforms) writes 4-byte elements, dtype %d is not 4 bytes wide", mode, dtype);
    const uintptr_t width = dtype == VAW_F64 ? 8 : dtype == VAW_BF16 ? 2 : 4;
    VAW_CHECK_ARG(((uintptr_t)out & (width - 1)) == 0 && ((uintptr_t)seeds & 7) == 0, "randn_seeded: pointer not aligned to its element");
    if (mode == VAW_NOISE_BITS) launch_randn_seeded<0, uint32_t>(out, seeds, B, per_sample, draw, tag, stream);
    else if (mode == VAW_NOISE_UNIFORM) launch_randn_seeded<1, float>(out, seeds, B, per_sample, draw, tag, stream);
    else if (dtype == VAW_F32) launch_randn_seeded<2, float>(out, seeds, B, per_sample, draw, tag, stream);
    else if (dtype == VAW_BF16) launch_randn_seeded<2, bf16_t>(out, seeds, B, per_sample, draw, tag, stream);
    else launch_randn_seeded<2, double>(out, seeds, B, per_sample, draw, tag, stream);
    VAW_CHECK_LAUNCH("randn_seeded");
    return VAW_OK;
}

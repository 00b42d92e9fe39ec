/*
 * fr_srgb.h — internal: the tables of LINEAR-LIGHT SUPERSAMPLING (include/fractal_hip.h) as the filter kernels use them.
 * Included inside an anonymous namespace, like fr_colour.h: each translation unit compiles its own copy into its own kernels.
 *
 * A workgroup stages both tables into 1 KiB of LDS once (srgb_stage, before a barrier of its own kernel): 512 uint16,
 * L[0 .. 255] and behind it T[0 .. 255] with T[0] = 0, so that E(m) — the number of k in 1 .. 255 with m >= T[k] — is the
 * largest k in 0 .. 255 with T[k] <= m: eight steps of a bisection (srgb_encode), no branch.
 */
#ifndef FR_SRGB_H
#define FR_SRGB_H

#include "fr_srgb_table.inc"

constexpr uint32_t kSrgbLdsWords = 512; /* uint16 words: L, then T with T[0] = 0 */

__device__ const uint16_t g_srgb_decode[256] = FR_SRGB_DECODE_INIT;
__device__ const uint16_t g_srgb_threshold[255] = FR_SRGB_THRESHOLD_INIT;

/* both tables into s_lt[kSrgbLdsWords]; the caller synchronises */
__device__ __forceinline__ void srgb_stage(uint16_t *s_lt, uint32_t tid, uint32_t threads) {
    for (uint32_t k = tid; k < kSrgbLdsWords; k += threads)
        s_lt[k] = k < 256u ? g_srgb_decode[k] : k == 256u ? (uint16_t)0 : g_srgb_threshold[k - 257u];
}

/* L[v] of a byte */
__device__ __forceinline__ uint32_t srgb_decode(const uint16_t *s_lt, uint32_t v) { return s_lt[v]; }

/* E(m), 0 <= m <= 65535 */
__device__ __forceinline__ uint32_t srgb_encode(const uint16_t *s_lt, uint32_t m) {
    const uint16_t *t = s_lt + 256;
    uint32_t k = 0;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1)
        if (t[k + step] <= m) k += step;
    return k;
}

#endif

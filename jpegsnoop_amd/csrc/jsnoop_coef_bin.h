// jsnoop_coef_bin.h -- the value part of one coefficient of jsnoop_batch_pack_coef_hist, shared by the host (records, tests/cpp/coef_hist_sweep.cpp) and
// k_coef_hist (jsnoop_coef_hist.hip): the division of an int16 arena value by its DQT entry, truncating toward zero as C's `/` does, and the clamp to a bin.
// Integer arithmetic only.  No hardware divide: |v| <= 32768 and q <= 65535, so with m = floor(2^31 / q) + 1 = (2^31 + e) / q, 0 < e <= q,
//   |v| * m / 2^31 = |v| / q + |v| * e / (q * 2^31), and |v| * e < 2^15 * 2^16 = 2^31 keeps the second term below 1 / q:
// the floor is floor(|v| / q).  2 |v| <= 2^16 and m <= 2^31 + 1 fit 32 bits, so the quotient is the high word of ONE 32 x 32 multiplication.
// q = 1 (dequantised rows) gives m = 2^31 + 1 and the value itself.  The sweep runs every v and every q against `/`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JS_BIN_FN __host__ __device__ inline
#else
#define JS_BIN_FN inline
#endif

// q = 0 (a table entry no decoder can divide by) counts as 1
JS_BIN_FN uint32_t js_chist_recip(uint32_t q) { return 0x80000000u / (q ? q : 1u) + 1u; }
JS_BIN_FN int32_t  js_chist_div(int32_t v, uint32_t m)
{
    const uint32_t n = (uint32_t)(v < 0 ? -v : v), x = (uint32_t)(((uint64_t)(n << 1) * m) >> 32);
    return v < 0 ? -(int32_t)x : (int32_t)x;
}
// bin of x under range r (1 .. 127): both end bins saturate
JS_BIN_FN uint32_t js_chist_bin(int32_t x, int32_t r) { return (uint32_t)((x < -r ? -r : (x > r ? r : x)) + r); }
// row length in words: 64 histograms of 2 r + 1 bins, 64 minima, 64 maxima
JS_BIN_FN uint32_t js_chist_words(uint32_t r) { return 64u * (2u * r + 1u) + 128u; }
// t / hv for t < 96, hv = 1 .. 16, magic = 65536 / hv + 1
JS_BIN_FN uint32_t js_chist_small_div(uint32_t t, uint32_t magic) { return (t * magic) >> 16; }

// jsnoop_carve.hip -- the kernels of jsnoop_carve_run: every FF D8 FF of a byte blob found, and the marker chain of each walked to its EOI, on the device
// (the definition: tests/carve_model.py; host side: jsnoop_carve.cpp; the walk itself and the sizes: jsnoop_carve_check.h).  Count, prefix sums, write -- export's shape.
//
// Coordinates: `base` is the 16-byte boundary at or below the blob's first byte, head = blob - base (0..15), end = head + n.  A position v counts from base, the
// blob's own position is v - head.  Every load is a whole aligned 16-byte piece that holds at least one byte of the blob (so it stays inside the blob's pages),
// whatever the blob's alignment; bits of bytes in front of the blob or behind it are masked off, which is all the peeling there is.
// A tile is CV_TILE bytes from a multiple of CV_TILE in these coordinates, the work of one workgroup of 256 threads: 4 rounds of 4 KiB, lane l of the workgroup taking
// bytes [16 l, 16 l + 16) of the round -- one global_load_dwordx4, 1 KiB contiguous per wave instruction, the four rounds' loads issued before the first use.
//
//   k_carve_count  per lane and round a 16-bit terminator mask and a 16-bit candidate mask (cv_masks: FF by SWAR compares on the four words, then the one or two
//                  bytes behind every FF, which for the piece's last bytes lie in the first word of the next piece -- from the neighbouring lane by a shuffle, for
//                  lane 63 from a second read); popcounts reduce to two counts per tile.
//   k_carve_scan   exclusive prefix sums of the tile counts (one workgroup, 16384 tiles a step, both counts in one 64-bit word) and the two totals.
//   k_carve_emit   the masks again; positions go to tile base + (round, wave) base + lane prefix of the two lists, so both lists ascend by construction -- no atomic
//                  decides an order.
//   k_carve_walk   one lane per candidate: js_carve_walk with byte reads from the blob and a binary search in the terminator list behind every SOS; one 64-byte
//                  record per candidate, four 16-byte stores.
#include <hip/hip_runtime.h>
#include "jsnoop_launch.h"
#include "jsnoop_carve_check.h"

#define CV_THREADS 256u
#define CV_ROUNDS  4u
#define CV_ROUND_BYTES (CV_THREADS * JS_CARVE_LANE)
#define CV_SCAN_THREADS 1024u
#define CV_SCAN_PER 16u
static_assert(JS_CARVE_WAVE == 64u * JS_CARVE_LANE && JS_CARVE_TILE == CV_ROUNDS * CV_ROUND_BYTES && JS_CARVE_WALK == CV_THREADS, "a lane owns 16 bytes of a round / a candidate");

typedef uint32_t cv_u32x4 __attribute__((ext_vector_type(4)));

// bit j = byte j of x equals the byte repeated in pat (exact: the 7-bit add cannot carry into the next byte)
__device__ __forceinline__ uint32_t cv_eq4(uint32_t x, uint32_t pat)
{
    const uint32_t y = x ^ pat, t = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;
    return (((~t & 0x80808080u) >> 7) * 0x10204080u) >> 28;
}
// the four bytes of the 20-byte window (the piece, then nx) from byte i on, i = 1 .. 16; what the shift brings in past byte 19 is never looked at
__device__ __forceinline__ uint32_t cv_window(const cv_u32x4 x, uint32_t nx, uint32_t i)
{
    const uint32_t w = i >> 2;
    const uint32_t lo = w == 0u ? x.x : w == 1u ? x.y : w == 2u ? x.z : w == 3u ? x.w : nx, hi = w == 0u ? x.y : w == 1u ? x.z : w == 2u ? x.w : nx;
    return __builtin_amdgcn_alignbyte(hi, lo, i & 3u);
}
// the piece at v (zero where it holds no byte of the blob) and the first word of the piece behind it
__device__ __forceinline__ cv_u32x4 cv_load(const uint8_t* __restrict__ base, uint64_t v, uint64_t end)
{
    cv_u32x4 x = { 0u, 0u, 0u, 0u };
    if (v < end) x = *reinterpret_cast<const cv_u32x4*>(base + v);
    return x;
}
__device__ __forceinline__ uint32_t cv_next(const uint8_t* __restrict__ base, uint64_t v, uint64_t end, uint32_t x0)
{
    uint32_t nx = __shfl_down(x0, 1);
    if ((threadIdx.x & 63u) == 63u) { nx = 0u; if (v + JS_CARVE_LANE < end) nx = *reinterpret_cast<const uint32_t*>(base + v + JS_CARVE_LANE); }
    return nx;
}
// tm bit k: v + k is a terminator; cm bit k: v + k is a candidate.  A terminator needs its next byte inside the blob (B past the end is 00), a candidate two.
// FF is found for all 16 bytes at once (SWAR compares); what follows an FF is looked at FF by FF: entropy-coded data has one FF in 256 bytes, so a wave's lanes
// go round this loop once or twice a piece, and a piece of nothing but FF sixteen times.
__device__ __forceinline__ void cv_masks(const cv_u32x4 x, uint32_t nx, uint64_t v, uint32_t head, uint64_t end, uint32_t& tm, uint32_t& cm)
{
    const uint32_t ff = cv_eq4(x.x, 0xFFFFFFFFu) | cv_eq4(x.y, 0xFFFFFFFFu) << 4 | cv_eq4(x.z, 0xFFFFFFFFu) << 8 | cv_eq4(x.w, 0xFFFFFFFFu) << 12;
    const uint32_t lo = v < head ? (0xFFFFu << (head - (uint32_t)v)) & 0xFFFFu : 0xFFFFu;
    const uint64_t room = end > v ? end - v : 0u;                                                                // bytes of the blob from v on
    const uint32_t tn = room > 1u ? (room - 1u > 16u ? 16u : (uint32_t)(room - 1u)) : 0u, cn = room > 2u ? (room - 2u > 16u ? 16u : (uint32_t)(room - 2u)) : 0u;
    uint32_t t = 0u, c = 0u;
    for (uint32_t m = ff & lo & ((1u << tn) - 1u); m; m &= m - 1u) {
        const uint32_t k = (uint32_t)__ffs(m) - 1u, next = cv_window(x, nx, k + 1u), b1 = next & 255u;
        if (b1 != 0u && (b1 & 0xF8u) != 0xD0u) t |= 1u << k;                                                     // neither 00 nor D0..D7
        if ((next & 0xFFFFu) == 0xFFD8u) c |= 1u << k;                                                           // D8, then FF
    }
    tm = t; cm = c & ((1u << cn) - 1u);
}

__global__ void __launch_bounds__(CV_THREADS) k_carve_count(const uint8_t* __restrict__ base, uint32_t head, uint64_t end, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_sum[2];
    const uint32_t t = threadIdx.x;
    const uint64_t v0 = (uint64_t)blockIdx.x * JS_CARVE_TILE + t * JS_CARVE_LANE;
    if (t < 2u) s_sum[t] = 0u;
    cv_u32x4 x[CV_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CV_ROUNDS; r++) x[r] = cv_load(base, v0 + r * CV_ROUND_BYTES, end);
    uint32_t ct = 0, cc = 0;
#pragma unroll
    for (uint32_t r = 0; r < CV_ROUNDS; r++) {
        const uint64_t v = v0 + r * CV_ROUND_BYTES;
        uint32_t tm, cm;
        cv_masks(x[r], cv_next(base, v, end, x[r].x), v, head, end, tm, cm);
        ct += __popc(tm); cc += __popc(cm);
    }
    for (uint32_t d = 32; d; d >>= 1) { ct += __shfl_xor(ct, d); cc += __shfl_xor(cc, d); }
    __syncthreads();
    if ((t & 63u) == 0u) { atomicAdd(&s_sum[0], ct); atomicAdd(&s_sum[1], cc); }                                 // (sums of integers: the order is immaterial)
    __syncthreads();
    if (t < 2u) counts[2u * blockIdx.x + t] = s_sum[t];
}

// counts: [tiles][2] counts, [tiles][2] exclusive prefix sums, then the totals as two 64-bit words.  One workgroup; a pair of counts is one 64-bit word, terminators
// low and candidates high (neither sum reaches 2^32, because n < 2^32).  A thread sums CV_SCAN_PER consecutive tiles on its own, the workgroup scans the threads' sums.
__global__ void __launch_bounds__(CV_SCAN_THREADS) k_carve_scan(unsigned long long* __restrict__ counts, uint32_t tiles)
{
    __shared__ unsigned long long s[CV_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t b = 0; b < tiles; b += CV_SCAN_THREADS * CV_SCAN_PER) {
        const uint32_t i0 = b + t * CV_SCAN_PER;
        unsigned long long before[CV_SCAN_PER], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < CV_SCAN_PER; j++) { before[j] = sum; if (i0 + j < tiles) sum += counts[i0 + j]; }
        s[t] = sum; __syncthreads();
        for (uint32_t d = 1; d < CV_SCAN_THREADS; d <<= 1) {
            const unsigned long long a = t >= d ? s[t - d] : 0ull; __syncthreads();
            s[t] += a; __syncthreads();
        }
        const unsigned long long excl = carry + s[t] - sum;
#pragma unroll
        for (uint32_t j = 0; j < CV_SCAN_PER; j++) if (i0 + j < tiles) counts[(size_t)tiles + i0 + j] = excl + before[j];
        carry += s[CV_SCAN_THREADS - 1u]; __syncthreads();
    }
    if (t == 0u) { counts[2u * (size_t)tiles] = carry & 0xFFFFFFFFull; counts[2u * (size_t)tiles + 1u] = carry >> 32; }
}

__global__ void __launch_bounds__(CV_THREADS) k_carve_emit(const uint8_t* __restrict__ base, uint32_t head, uint64_t end, const uint32_t* __restrict__ pre /*[tiles][2]*/,
                                                           uint32_t nterm, uint32_t ncand, uint32_t* __restrict__ term, uint32_t* __restrict__ cand)
{
    __shared__ uint32_t s_part[CV_ROUNDS * 4u];                     // sums of (round, wave), terminators low, candidates high: a tile holds at most 16384 of each
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t v0 = (uint64_t)blockIdx.x * JS_CARVE_TILE + t * JS_CARVE_LANE;
    cv_u32x4 x[CV_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CV_ROUNDS; r++) x[r] = cv_load(base, v0 + r * CV_ROUND_BYTES, end);
    uint32_t tm[CV_ROUNDS], cm[CV_ROUNDS], before[CV_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CV_ROUNDS; r++) {
        const uint64_t v = v0 + r * CV_ROUND_BYTES;
        cv_masks(x[r], cv_next(base, v, end, x[r].x), v, head, end, tm[r], cm[r]);
        const uint32_t own = (uint32_t)__popc(tm[r]) | (uint32_t)__popc(cm[r]) << 16;
        uint32_t incl = own;
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t a = __shfl_up(incl, d); if (lane >= d) incl += a; }
        before[r] = incl - own;
        if (lane == 63u) s_part[r * 4u + wave] = incl;
    }
    __syncthreads();
    const uint32_t tb = pre[2u * blockIdx.x], cb = pre[2u * blockIdx.x + 1u];
#pragma unroll
    for (uint32_t r = 0; r < CV_ROUNDS; r++) {
        uint32_t part = 0;
        for (uint32_t q = 0; q < r * 4u + wave; q++) part += s_part[q];
        part += before[r];
        const uint32_t p0 = (uint32_t)(v0 + r * CV_ROUND_BYTES - head);       // the blob's position of bit 0 (never used for a masked bit)
        uint32_t ti = tb + (part & 0xFFFFu), ci = cb + (part >> 16);
        for (uint32_t m = tm[r]; m; m &= m - 1u) { if (ti < nterm) term[ti] = p0 + (uint32_t)__ffs(m) - 1u; ti++; }
        for (uint32_t m = cm[r]; m; m &= m - 1u) { if (ci < ncand) cand[ci] = p0 + (uint32_t)__ffs(m) - 1u; ci++; }
    }
}

struct CvAt {
    const uint8_t* blob; uint64_t n;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return i < n ? blob[i] : 0u; }
};
struct CvNext {                                                      // the least terminator >= pos, or UINT64_MAX
    const uint32_t* term; uint32_t nterm;
    __device__ __forceinline__ uint64_t operator()(uint64_t pos) const
    {
        uint32_t lo = 0, hi = nterm;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)term[mid] < pos) lo = mid + 1u; else hi = mid; }
        return lo < nterm ? (uint64_t)term[lo] : UINT64_MAX;
    }
};
__global__ void __launch_bounds__(CV_THREADS) k_carve_walk(const uint8_t* __restrict__ blob, uint64_t n, const uint32_t* __restrict__ term, uint32_t nterm,
                                                           const uint32_t* __restrict__ cand, uint32_t ncand, uint32_t max_markers, cv_u32x4* __restrict__ recs)
{
    const uint32_t k = blockIdx.x * CV_THREADS + threadIdx.x;
    if (k >= ncand) return;
    JsCarveRec r;
    js_carve_walk(n, cand[k], max_markers, CvAt{ blob, n }, CvNext{ term, nterm }, &r);
#pragma unroll
    for (uint32_t q = 0; q < JS_CARVE_REC_WORDS / 4u; q++) {
        const cv_u32x4 o = { r.w[4u * q], r.w[4u * q + 1u], r.w[4u * q + 2u], r.w[4u * q + 3u] };
        recs[(size_t)k * (JS_CARVE_REC_WORDS / 4u) + q] = o;
    }
}

int js_launch_carve_count(hipStream_t st, const uint8_t* base, uint32_t head, uint64_t n, uint32_t tiles, uint32_t* counts)
{
    if (tiles) k_carve_count<<<tiles, CV_THREADS, 0, st>>>(base, head, (uint64_t)head + n, counts);
    k_carve_scan<<<1, CV_SCAN_THREADS, 0, st>>>(reinterpret_cast<unsigned long long*>(counts), tiles);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int js_launch_carve_walk(hipStream_t st, const uint8_t* base, uint32_t head, uint64_t n, uint32_t tiles, const uint32_t* counts, uint32_t nterm, uint32_t ncand,
                         uint32_t max_markers, uint32_t* term, uint32_t* cand, uint32_t* recs)
{
    if (tiles && (nterm || ncand)) k_carve_emit<<<tiles, CV_THREADS, 0, st>>>(base, head, (uint64_t)head + n, counts + 2u * (size_t)tiles, nterm, ncand, term, cand);
    if (ncand) k_carve_walk<<<(ncand + CV_THREADS - 1u) / CV_THREADS, CV_THREADS, 0, st>>>(base + head, n, term, nterm, cand, ncand, max_markers, reinterpret_cast<cv_u32x4*>(recs));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

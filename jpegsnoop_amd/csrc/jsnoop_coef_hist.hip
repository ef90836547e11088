// jsnoop_coef_hist.hip -- k_coef_hist: the histogram of every DCT frequency of any list of (image, component) pairs of a decoded batch, one row of
// 64 * NB + 128 words (NB = 2 R + 1 bins; then 64 minima, 64 maxima) per pair in caller-owned device memory.
//
// The value of block b at natural index k is the arena's int16 (k = 0: the cumulative DC of the dccum arena), divided by the DQT entry of k where the row
// asks for quantised levels: js_chist_div / js_chist_bin of jsnoop_coef_bin.h, the text the host sweep runs over every value and divisor.  Everything else
// is an integer min, max or add, which no order of evaluation changes.
//
// Work: ONE launch for the whole list behind k_coef_hist_init, which sets the rows (counts 0, minima INT32_MAX, maxima INT32_MIN).  A unit is a run of up to
// JS_COEF_HIST_UNIT = 64 of a component's blocks in ARENA order, done by one wave with k_pack_coefs' loads: eight lanes a block, a lane reads 16 bytes (eight
// coefficients) of each of eight blocks -- eight loads in flight before the arithmetic -- and the lane that owns natural index 0 swaps in the dccum value.
// Units are numbered through a 64-bit prefix table over the records and dealt like k_pack_coefs': a workgroup takes a contiguous share and finds the record
// of its first unit by one search.  The share is walked destination by destination (the bounds are workgroup-uniform and live in scalar registers); inside
// one destination its eight waves interleave.
//
// Histograms: ONE per workgroup of eight waves in LDS, 64 * NB words (R = 127: 65 280 bytes), filled with ds_add_u32 whose result is not used.  Two workgroups
// a CU at every R: sixteen waves, four a SIMD -- with four-wave workgroups the LDS of R = 127 left two waves a SIMD, and the call, whose waves load, wait
// and then compute, took half as long again.  Zeros are 85 % of a natural picture's coefficients and never reach LDS: a lane skips x == 0, and the zero bin of a position is
// rebuilt at the flush as (blocks counted) - (sum of its other bins) -- for R >= 1 the zero bin is none of the clamp bins.  Rows of consecutive positions
// start NB words apart and NB is odd, so the same bin of neighbouring positions lies in different banks.
// Minima and maxima of a lane's eight positions stay in registers across its units of one destination.
// Flush (the share moves to the next destination, or ends): the workgroup meets, eight threads a position sum the other bins and write the zero bin, then
// all 512 threads sweep the histogram -- consecutive lanes, consecutive words -- and add what is not zero to the row with global integer atomics whose
// result is not used, leaving zeros behind.  Every wave reduces its extrema over the eight lanes that share positions, moves them so that lane L holds
// natural index L, and sends one atomic min and one atomic max per lane.
//
// Stores to device memory: vector stores (the init) and atomics only.  No scratch memory.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_coef_bin.h"

#define CH_WAVES   JS_COEF_HIST_WAVES
#define CH_THREADS (CH_WAVES * 64u)
#define CH_LDS_PER_CU 163840u
#define CH_WAVES_PER_SIMD (CH_WAVES * JS_COEF_HIST_WG_PER_CU / 4u)          /* the occupancy the registers are held to: 128 VGPRs */

typedef uint32_t ch_u32x4 __attribute__((ext_vector_type(4)));
#define CH_GLOBAL __attribute__((address_space(1)))

__constant__ uint8_t c_ch_position[64] = JS_ZIGZAG_POSITION;

__global__ void __launch_bounds__(CH_THREADS) k_coef_hist_init(uint32_t* __restrict__ dst, uint64_t pitch_words, uint32_t hist_words)
{
    const uint32_t w = blockIdx.y * CH_THREADS + threadIdx.x;                        // row blockIdx.x
    if (w >= hist_words + 128u) return;
    dst[(size_t)blockIdx.x * pitch_words + w] = w < hist_words ? 0u : (w < hist_words + 64u ? 0x7FFFFFFFu : 0x80000000u);
}

template <int ORDER>
__global__ void __launch_bounds__(CH_THREADS, CH_WAVES_PER_SIMD) k_coef_hist(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsCoefHistRec* __restrict__ recs,
                                                          const uint64_t* __restrict__ unit_base, uint32_t nrec, uint64_t total_units, uint64_t units_per_wg, int range)
{
    extern __shared__ uint32_t s_hist[];                                             // [64][NB]
    const uint32_t t = threadIdx.x, lane = t & 63u, hi = lane >> 3, lo = lane & 7u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t nb = 2u * (uint32_t)range + 1u, hist_words = 64u * nb;
    // this workgroup's share of the units: [u0, u1)  (the host sized the grid: no product here passes total_units + units_per_wg)
    const uint64_t u0 = (uint64_t)blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);
    if (u0 >= u1) return;
    for (uint32_t i = t; i < hist_words; i += CH_THREADS) s_hist[i] = 0u;
    // the zero bin of each of this lane's eight natural indices 8 lo .. 8 lo + 7
    uint32_t hb[8];
    #pragma unroll
    for (int e = 0; e < 8; e++) { const uint32_t nat = lo * 8u + e; hb[e] = (ORDER == JSNOOP_COEF_ZIGZAG ? (uint32_t)c_ch_position[nat] : nat) * nb + (uint32_t)range; }
    const uint32_t my_pos = ORDER == JSNOOP_COEF_ZIGZAG ? (uint32_t)c_ch_position[lane] : lane;      // at the flush lane L speaks for natural index L
    // the record of the first unit: the last k with unit_base[k] <= u0 (unit_base[0] = 0, unit_base[nrec] = total_units > u0)
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u0) k = mid; else top = mid; }
    __syncthreads();
    for (uint64_t s0 = u0; s0 < u1; ) {
        while (s0 >= unit_base[k + 1]) k++;
        const uint64_t kbeg = unit_base[k], s1 = min(u1, unit_base[k + 1]);
        const JsCoefHistRec* r = recs + k;
        const uint64_t coef_off = r->coef_off; const uint32_t nblk = r->nblk, hv = r->hv, first = r->first, bpm = r->bpm, hv_magic = r->hv_magic;
        CH_GLOBAL uint32_t* dst = reinterpret_cast<CH_GLOBAL uint32_t*>(r->dst);
        const ch_u32x4 ma = *reinterpret_cast<const ch_u32x4*>(r->recip + lo * 8u), mb = *reinterpret_cast<const ch_u32x4*>(r->recip + lo * 8u + 4u);
        const uint32_t m[8] = { ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w };
        int mn[8], mx[8];
        #pragma unroll
        for (int e = 0; e < 8; e++) { mn[e] = 0x7FFFFFFF; mx[e] = (int)0x80000000; }
        const uint32_t lu0 = (uint32_t)(s0 - kbeg), lu1 = (uint32_t)(s1 - kbeg);     // units of this destination: nblk < 2^32 blocks
        for (uint32_t lu = lu0 + wave; lu < lu1; lu += CH_WAVES) {
            const uint32_t n0 = lu * JS_COEF_HIST_UNIT, cnt = min(JS_COEF_HIST_UNIT, nblk - n0);
            const uint32_t m0 = n0 / hv, j0 = n0 - m0 * hv;
            const uint64_t blk0 = coef_off + (uint64_t)m0 * bpm + first;
            // ---- load: pass p takes blocks 8 p .. 8 p + 7 of the run, lane (hi, lo) chunk lo of block 8 p + hi
            ch_u32x4 v[8];
            #pragma unroll
            for (int p = 0; p < 8; p++) {
                const uint32_t o = p * 8u + hi;
                v[p] = ch_u32x4{ 0u, 0u, 0u, 0u };
                if (o < cnt) {
                    const uint32_t tt = j0 + o, dm = js_chist_small_div(tt, hv_magic);
                    const uint64_t blk = blk0 + (uint64_t)dm * bpm + (tt - dm * hv);
                    v[p] = *reinterpret_cast<const ch_u32x4*>(coef + blk * 64u + lo * 8u);
                    if (lo == 0u) v[p].x = (v[p].x & 0xFFFF0000u) | (uint32_t)(uint16_t)dccum[blk];
                }
            }
            #pragma unroll
            for (int p = 0; p < 8; p++) {
                if (p * 8u + hi < cnt) {
                    const uint32_t w[4] = { v[p].x, v[p].y, v[p].z, v[p].w };
                    #pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const int val = (e & 1) ? (int)w[e >> 1] >> 16 : (int)(int16_t)w[e >> 1];
                        const int x = js_chist_div(val, m[e]);
                        mn[e] = min(mn[e], x); mx[e] = max(mx[e], x);
                        if (x != 0) atomicAdd(&s_hist[hb[e] + (uint32_t)min(max(x, -range), range)], 1u);
                    }
                }
            }
        }
        __syncthreads();
        // ---- flush: the zero bins, then the histogram, then the extrema
        const uint32_t blocks = min(lu1 * JS_COEF_HIST_UNIT, nblk) - lu0 * JS_COEF_HIST_UNIT;
        {
            const uint32_t p = t >> 3, part = t & 7u; uint32_t* row = s_hist + p * nb;      // CH_THREADS / 64 = 8 threads a position
            uint32_t s = 0;
            for (uint32_t b = part; b < nb; b += 8u) s += row[b];                    // (the zero bin holds 0)
            s += (uint32_t)__shfl_xor((int)s, 1); s += (uint32_t)__shfl_xor((int)s, 2); s += (uint32_t)__shfl_xor((int)s, 4);
            if (part == 0u) row[(uint32_t)range] = blocks - s;
        }
        __syncthreads();
        for (uint32_t i = t; i < hist_words; i += CH_THREADS) { const uint32_t c = s_hist[i]; if (c) { __hip_atomic_fetch_add(dst + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); s_hist[i] = 0u; } }
        if (lu0 + wave < lu1) {                                                      // (wave-uniform: a wave without a unit holds the seeds)
            int mnv = 0x7FFFFFFF, mxv = (int)0x80000000;
            #pragma unroll
            for (int e = 0; e < 8; e++) {
                int a = mn[e], b = mx[e];
                #pragma unroll
                for (int o = 8; o < 64; o <<= 1) { a = min(a, __shfl_xor(a, o)); b = max(b, __shfl_xor(b, o)); }
                a = __shfl(a, (int)(lane >> 3)); b = __shfl(b, (int)(lane >> 3));   // lane L takes natural index L = 8 lo' + e from a lane whose lo is lo'
                if ((lane & 7u) == (uint32_t)e) { mnv = a; mxv = b; }
            }
            __hip_atomic_fetch_min(reinterpret_cast<CH_GLOBAL int*>(dst) + hist_words + my_pos, mnv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(reinterpret_cast<CH_GLOBAL int*>(dst) + hist_words + 64u + my_pos, mxv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        s0 = s1;
    }
}

// k_coef_hist_init, then k_coef_hist: JS_COEF_HIST_WG_PER_CU workgroups per compute unit of the CURRENT device (fewer if the LDS held fewer histograms), never
// more workgroups than there are steps of JS_COEF_HIST_WAVES units.  0, -1 on a launch error or an unknown order / range.
int js_launch_coef_hist(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsCoefHistRec* recs, const uint64_t* unit_base, uint32_t nrec, uint64_t total_units,
                        int order, uint32_t range, void* dst, uint64_t pitch_words)
{
    if (!nrec || !total_units) return 0;
    if ((order | 1) != 1 || range < 1u || range > 127u) return -1;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint32_t hist_words = 64u * (2u * range + 1u), lds = hist_words * 4u;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * std::min(JS_COEF_HIST_WG_PER_CU, CH_LDS_PER_CU / lds), (total_units + CH_WAVES - 1u) / CH_WAVES);
    const uint64_t units_per_wg = (total_units + want - 1u) / want, grid = (total_units + units_per_wg - 1u) / units_per_wg;
    if (grid > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(k_coef_hist_init, dim3(nrec, (hist_words + 128u + CH_THREADS - 1u) / CH_THREADS), dim3(CH_THREADS), 0, st, static_cast<uint32_t*>(dst), pitch_words, hist_words);
    if (order == JSNOOP_COEF_ZIGZAG)
        hipLaunchKernelGGL(k_coef_hist<JSNOOP_COEF_ZIGZAG>, dim3((uint32_t)grid), dim3(CH_THREADS), lds, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, (int)range);
    else
        hipLaunchKernelGGL(k_coef_hist<JSNOOP_COEF_NATURAL>, dim3((uint32_t)grid), dim3(CH_THREADS), lds, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, (int)range);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

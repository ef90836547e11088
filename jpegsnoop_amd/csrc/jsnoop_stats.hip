// jsnoop_stats.hip -- k_stats_batch / k_stats_order: the bHistoEn / bStatClipEn colour statistics of any subset of a decoded batch, one row of
// JSNOOP_STATS_WORDS words per listed image in caller-owned device memory, in two launches and without a host decision in between.
//
// Every row holds what k_color_stats / k_clip_order and the budget logic of JsnoopBatch::color_stats_pass leave for that image alone: the per-pixel
// arithmetic is stat_values of jsnoop_stat_pixel.h, the one those kernels use, and everything else is an integer min, max or add, which no order of
// evaluation changes.
//
// k_stats_batch<HIST>.  A unit is a run of up to JS_STATS_UNIT = 512 pixels of one row of the MCU-padded picture, done by one wave: a lane owns eight
// consecutive samples and loads them as ONE 16-byte vector per plane (rows, plane_off and plane sizes are multiples of eight samples: every load is aligned;
// a wave-load covers 1 KiB of a plane row), the loads of all three planes in flight before the arithmetic.  Units are numbered through a 64-bit prefix table
// over the records (unit_base, nrec + 1 entries) and dealt like k_pack_coefs': a workgroup takes a contiguous share, its four waves interleaved, finds the
// record of its first unit by one search and walks on from there; what depends on the unit alone is wave-uniform and lives in scalar registers.
// Records, clip counters and event totals stay in registers across a wave's units of one destination; the three 128-bin histograms and the 2048-bin Y
// histogram are WAVE-PRIVATE in LDS (ds_add_u32 without return; 9.5 KiB a wave, four workgroups a CU), so no wave ever waits for another.  When a wave's
// share moves to the next destination, and at its end, it flushes: registers reduced across the wave, staged through LDS so that consecutive lanes address
// consecutive words, and added to the zeroed destination row with global integer atomics whose result is not used (no-return form); histogram bins in
// runs of 64 consecutive words, zero values skipped, the Y histogram only between the bins of the smallest and the largest Y the wave saw.
// Besides the row, in batch scratch: the six range-event totals of every row (tot, JS_STATS_TOT_WORDS apart) and the number of range events of every picture
// row (rowcnt, from record.row_base on) -- one atomic add per unit that saw an event, none from the others.  The kernel is bound by VALU issue, so a pixel's twelve range counters sit behind ONE test of its six values, and the ClipRGB records are derived from the PreclipRGB ones at the flush.
//
// k_stats_order.  One workgroup per listed row.  The reference counts a YCC range event only while fewer than 10 were reported (CapYccRange :4372-4378),
// in visiting order: raster order, within a pixel Y over, Y under, Cb over, Cb under, Cr over, Cr under.  A row whose total is at most 10 takes its totals
// as words 37..42.  Otherwise the workgroup scans the per-row counts for the picture rows that hold events 0..9 -- at most ten rows, each with the ordinal
// of its first event -- and its waves walk only those rows, a prefix count over 64 pixels a step, and count by kind the events whose ordinal is below 10.
// Its work is bounded by the picture's height plus ten row widths.
//
// Stores to device memory: vector stores and atomics only.  No scratch memory in any instance.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_stat_pixel.h"

#define SB_THREADS 256
#define SB_WAVES   (SB_THREADS / 64)
#define SB_HIST_WORDS (3u * 128u + 2048u)            /* LDS words of one wave's histograms: R, G, B, then Y */
#define SB_BUDGET 10u                                 /* YCC_CLIP_REPORT_MAX */

typedef uint32_t sb_u32x4 __attribute__((ext_vector_type(4)));

struct SbShift { int shift_y, shift_cb, shift_cr; };
struct SbAcc { int mn[12], mx[12]; uint32_t sm[12], clip[6], tot[6], fix[3], n; };     // fix: sum of (lim - rgb), what the ClipRGB sums lack of the PreclipRGB sums

__device__ __forceinline__ void sb_clear(SbAcc& a)
{
    #pragma unroll
    for (int i = 0; i < 12; i++) { a.mn[i] = 0; a.mx[i] = 0; a.sm[i] = 0; }       // the reference's records start from memset(0) (:3146-3147)
    #pragma unroll
    for (int i = 0; i < 6; i++) { a.clip[i] = 0; a.tot[i] = 0; }
    a.fix[0] = a.fix[1] = a.fix[2] = 0; a.n = 0;
}
__device__ __forceinline__ int      sb_wave_min(int v)      { for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int      sb_wave_max(int v)      { for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ uint32_t sb_wave_add(uint32_t v) { for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o); return v; }
__device__ __forceinline__ void sb_wave_sync()
{ __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// What one wave holds for destination row `dst` (record k) goes out; registers and histograms are back at zero afterwards.
template <bool HIST>
__device__ __forceinline__ void sb_flush(SbAcc& a, uint32_t* __restrict__ hist, uint32_t* __restrict__ stage, uint32_t lane, uint32_t* __restrict__ dst, uint32_t* __restrict__ tot_k)
{
    if (HIST) {
        #pragma unroll
        for (int i = 0; i < 12; i++) { a.mn[i] = sb_wave_min(a.mn[i]); a.mx[i] = sb_wave_max(a.mx[i]); a.sm[i] = sb_wave_add(a.sm[i]); }
        a.n = sb_wave_add(a.n);
        // ClipRGB (groups 6-8) from PreclipRGB (9-11): rgb = clamp(lim, 0, 255) is monotonic, so its extremes are the clamped extremes (the minimum of values >= 0 under
        // a seed of 0 is 0), and its sum is lim's less what the clipped samples lost -- gathered where a sample leaves a range, nowhere else
        #pragma unroll
        for (int c = 0; c < 3; c++) { a.mn[6 + c] = 0; a.mx[6 + c] = min(a.mx[9 + c], 255); a.sm[6 + c] = a.sm[9 + c] - sb_wave_add(a.fix[c]); }
    }
    #pragma unroll
    for (int i = 0; i < 6; i++) { a.clip[i] = sb_wave_add(a.clip[i]); a.tot[i] = sb_wave_add(a.tot[i]); }
    if (lane == 0) {                                              // the row's layout: [0..35] records, [36] count, [37..42] <- the totals' place, [43..48] RGB clip counters
        #pragma unroll
        for (int i = 0; i < 12; i++) { stage[3 * i] = (uint32_t)a.mn[i]; stage[3 * i + 1] = (uint32_t)a.mx[i]; stage[3 * i + 2] = a.sm[i]; }
        stage[36] = a.n;
        #pragma unroll
        for (int i = 0; i < 6; i++) { stage[37 + i] = a.tot[i]; stage[43 + i] = a.clip[i]; }
    }
    sb_wave_sync();
    if (lane < 49) {
        const uint32_t v = stage[lane];
        if (v != 0u) {                                            // (a minimum is never above 0, a maximum never below: 0 changes nothing)
            if (lane < 36) {
                const uint32_t m = lane % 3u;
                if (m == 0u) atomicMin(reinterpret_cast<int*>(dst) + lane, (int)v);
                else if (m == 1u) atomicMax(reinterpret_cast<int*>(dst) + lane, (int)v);
                else atomicAdd(dst + lane, v);
            }
            else if (lane >= 37 && lane < 43) atomicAdd(tot_k + (lane - 37u), v);       // the budget is k_stats_order's business
            else atomicAdd(dst + lane, v);
        }
    }
    if (HIST) {
        #pragma unroll
        for (uint32_t i = 0; i < 384u; i += 64u) { const uint32_t v = hist[i + lane]; if (v) { atomicAdd(dst + 50u + i + lane, v); hist[i + lane] = 0u; } }
        const uint32_t lo = (uint32_t)(min(max(a.mn[0], -1024), 1023) + 1024) & ~63u, hi = (uint32_t)(min(max(a.mx[0], -1024), 1023) + 1024);
        for (uint32_t i = lo; i <= hi; i += 64u) { const uint32_t v = hist[384u + i + lane]; if (v) { atomicAdd(dst + 434u + i + lane, v); hist[384u + i + lane] = 0u; } }
    }
    sb_wave_sync();
    sb_clear(a);
}

template <bool HIST>
__global__ void __launch_bounds__(SB_THREADS) k_stats_batch(const int16_t* __restrict__ planes, const JsStatRec* __restrict__ recs, const uint64_t* __restrict__ unit_base,
                                                            uint32_t nrec, uint64_t total_units, uint64_t units_per_wg, uint32_t* __restrict__ tot, uint32_t* __restrict__ rowcnt)
{
    __shared__ uint32_t s_hist[HIST ? SB_WAVES * SB_HIST_WORDS : 1u];
    __shared__ uint32_t s_stage[SB_WAVES * 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* hist = s_hist + (HIST ? wave * SB_HIST_WORDS : 0u);
    uint32_t* stage = s_stage + wave * 64u;
    // this workgroup's share of the units: [u0, u1)  (the host sized the grid: no product here passes total_units + units_per_wg)
    const uint64_t u0 = (uint64_t)blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);
    uint64_t u = u0 + wave;
    if (u >= u1) return;
    if (HIST) { for (uint32_t i = lane; i < SB_HIST_WORDS; i += 64u) hist[i] = 0u; sb_wave_sync(); }
    // the record of the first unit: the last k with unit_base[k] <= u (unit_base[0] = 0, unit_base[nrec] = total_units > u)
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u) k = mid; else top = mid; }
    uint64_t kbeg = 0, kend = 0, psz = 0, row_base = 0; bool have = false;
    uint32_t img_x = 0, pw = 0, ncomp = 0, mcu_w = 8, mcu_h = 8, across = 0, shift_ind = 0, tiles = 1; SbShift sh = { 0, 0, 0 };
    const int16_t* pl = planes; uint32_t* dst = nullptr;
    SbAcc a; sb_clear(a);
    for (; u < u1; u += SB_WAVES) {
        if (!have || u >= kend) {
            if (have) sb_flush<HIST>(a, hist, stage, lane, dst, tot + (size_t)k * JS_STATS_TOT_WORDS);
            while (u >= unit_base[k + 1]) k++;
            have = true; kbeg = unit_base[k]; kend = unit_base[k + 1];
            const JsStatRec r = recs[k];
            dst = reinterpret_cast<uint32_t*>(r.dst); pl = planes + r.plane_off; psz = r.psz; row_base = r.row_base;
            img_x = r.img_x; pw = r.pw; ncomp = r.ncomp; mcu_w = r.mcu_w; mcu_h = r.mcu_h; across = r.across; shift_ind = r.shift_ind; tiles = r.tiles;
            sh.shift_y = r.shift_y; sh.shift_cb = r.shift_cb; sh.shift_cr = r.shift_cr;
        }
        const uint32_t lu = (uint32_t)(u - kbeg), py = lu / tiles, x0 = (lu - py * tiles) * JS_STATS_UNIT + lane * 8u;
        const bool active = x0 < img_x;                          // (img_x is a multiple of 8: a lane's eight samples are inside the row or none is)
        // ---- load: all planes in flight before the arithmetic
        sb_u32x4 vy = { 0u, 0u, 0u, 0u }, vcb = { 0u, 0u, 0u, 0u }, vcr = { 0u, 0u, 0u, 0u };
        if (active) {
            const int16_t* p = pl + (size_t)py * pw + x0;
            vy = *reinterpret_cast<const sb_u32x4*>(p);
            if (ncomp == 3u) { vcb = *reinterpret_cast<const sb_u32x4*>(p + psz); vcr = *reinterpret_cast<const sb_u32x4*>(p + 2u * psz); }   // one component: Cb = Cr = 0 (:4709-4715)
        }
        uint32_t evu = 0;
        if (active) {
            const bool shifted = (py / mcu_h) * across + x0 / mcu_w >= shift_ind;     // (mcu_w is a multiple of 8: the eight samples share their MCU)
            #pragma unroll 1
            for (int h = 0; h < 2; h++) {                        // two halves of four samples, not unrolled: the live values of eight samples at once cost a wave per SIMD
                const uint32_t wy[2] = { h ? vy.z : vy.x, h ? vy.w : vy.y }, wcb[2] = { h ? vcb.z : vcb.x, h ? vcb.w : vcb.y }, wcr[2] = { h ? vcr.z : vcr.x, h ? vcr.w : vcr.y };
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    StatPix q;
                    q.pre[0] = (int)(int16_t)(wy[j >> 1] >> (16 * (j & 1))); q.pre[1] = (int)(int16_t)(wcb[j >> 1] >> (16 * (j & 1))); q.pre[2] = (int)(int16_t)(wcr[j >> 1] >> (16 * (j & 1)));
                    stat_values(q, shifted, sh);
                    // a sample outside a range is rare: ONE test for all six values (in range = no bit above the low eight), the twelve counters only behind it
                    if ((uint32_t)(q.clipv[0] | q.clipv[1] | q.clipv[2] | q.lim[0] | q.lim[1] | q.lim[2]) > 255u) {
                        #pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const uint32_t un = q.clipv[c] < 0, ov = q.clipv[c] > 255;
                            a.tot[2 * c] += un; a.tot[2 * c + 1] += ov; evu += un + ov;
                            a.clip[2 * c] += q.lim[c] < 0; a.clip[2 * c + 1] += q.lim[c] > 255;     // RGB clip counters are unconditional (:4532-4586)
                            if (HIST) a.fix[c] += (uint32_t)(q.lim[c] - q.rgb[c]);
                        }
                    }
                    if (HIST) {
                        #pragma unroll
                        for (int c = 0; c < 3; c++) {                  // PixelCcHisto groups: PreclipYCC 0-2, ClipYCC 3-5, PreclipRGB 9-11; ClipRGB 6-8 at the flush
                            a.mn[c] = min(a.mn[c], q.pre[c]); a.mx[c] = max(a.mx[c], q.pre[c]); a.sm[c] += (uint32_t)q.pre[c];
                            a.mn[3 + c] = min(a.mn[3 + c], q.clipv[c]); a.mx[3 + c] = max(a.mx[3 + c], q.clipv[c]); a.sm[3 + c] += (uint32_t)q.clipv[c];
                            a.mn[9 + c] = min(a.mn[9 + c], q.lim[c]); a.mx[9 + c] = max(a.mx[9 + c], q.lim[c]); a.sm[9 + c] += (uint32_t)q.lim[c];
                            atomicAdd(&hist[c * 128 + (uint32_t)q.rgb[c] / 2u], 1u);        // 256 / HISTO_BINS = 2 (:4313-4317)
                        }
                        atomicAdd(&hist[384 + (uint32_t)(min(max(q.pre[0], -1024), 1023) + 1024)], 1u);   // m_anHistoYFull (:4254-4259)
                    }
                }
            }
            if (HIST) a.n += 8u;
        }
        if (__ballot(evu != 0u)) {                               // range events per picture row: only a unit that saw one adds
            const uint32_t s = sb_wave_add(evu);
            if (lane == 0) atomicAdd(rowcnt + row_base + py, s);
        }
    }
    sb_flush<HIST>(a, hist, stage, lane, dst, tot + (size_t)k * JS_STATS_TOT_WORDS);
}

// bit 2c: component c over, bit 2c + 1: component c under -- the order of CapYccRange's checks
__device__ __forceinline__ uint32_t sb_pixel_events(const int16_t* __restrict__ pl, const JsStatRec& r, uint32_t px, uint32_t py)
{
    const size_t pi = (size_t)py * r.pw + px;
    StatPix q;
    q.pre[0] = pl[pi]; q.pre[1] = r.ncomp == 3u ? pl[r.psz + pi] : 0; q.pre[2] = r.ncomp == 3u ? pl[2u * r.psz + pi] : 0;
    stat_values(q, (py / r.mcu_h) * r.across + px / r.mcu_w >= r.shift_ind, r);
    uint32_t ev = 0;
    #pragma unroll
    for (int c = 0; c < 3; c++) ev |= (q.clipv[c] > 255 ? 1u : 0u) << (2 * c) | (q.clipv[c] < 0 ? 2u : 0u) << (2 * c);
    return ev;
}
__device__ __forceinline__ uint32_t sb_wave_scan(uint32_t v, uint32_t lane)      // inclusive
{ for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)v, o); if (lane >= o) v += t; } return v; }

__global__ void __launch_bounds__(SB_THREADS) k_stats_order(const int16_t* __restrict__ planes, const JsStatRec* __restrict__ recs, const uint32_t* __restrict__ tot,
                                                            const uint32_t* __restrict__ rowcnt, uint32_t* __restrict__ totals_out)
{
    __shared__ uint32_t s_wave[SB_WAVES], s_row[SB_BUDGET], s_ord[SB_BUDGET], s_out[6], s_n;
    const uint32_t k = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const JsStatRec r = recs[k];
    uint32_t* dst = reinterpret_cast<uint32_t*>(r.dst);
    const uint32_t* tk = tot + (size_t)k * JS_STATS_TOT_WORDS;
    uint32_t total = 0;
    #pragma unroll
    for (int i = 0; i < 6; i++) total += tk[i];
    if (totals_out && t < 6) totals_out[(size_t)k * 6u + t] = tk[t];
    if (total <= SB_BUDGET) { if (t < 6) dst[37 + t] = tk[t]; return; }          // (the whole workgroup takes the same way)
    if (t < 6) s_out[t] = 0;
    if (t == 0) s_n = 0;
    __syncthreads();
    // the picture rows that hold events 0 .. 9, each with the ordinal of its first event
    const uint32_t* rc = rowcnt + r.row_base;
    uint32_t run = 0;
    for (uint32_t base = 0; base < r.img_y && run < SB_BUDGET; base += SB_THREADS) {
        const uint32_t c = base + t < r.img_y ? rc[base + t] : 0u, incl = sb_wave_scan(c, lane);
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        #pragma unroll
        for (uint32_t w = 0; w < SB_WAVES; w++) { const uint32_t v = s_wave[w]; all += v; if (w < wave) before += v; }
        const uint32_t first = run + before + incl - c;
        if (c && first < SB_BUDGET) { const uint32_t i = atomicAdd(&s_n, 1u); if (i < SB_BUDGET) { s_row[i] = base + t; s_ord[i] = first; } }
        run += all;
        __syncthreads();
    }
    const uint32_t n = min(s_n, SB_BUDGET);
    const int16_t* pl = planes + r.plane_off;
    for (uint32_t e = wave; e < n; e += SB_WAVES) {              // rows are independent once their first ordinal is known
        const uint32_t py = s_row[e];
        uint32_t ord0 = s_ord[e];
        for (uint32_t x0 = 0; x0 < r.img_x && ord0 < SB_BUDGET; x0 += 64u) {
            const uint32_t px = x0 + lane, ev = px < r.img_x ? sb_pixel_events(pl, r, px, py) : 0u, cnt = (uint32_t)__builtin_popcount(ev);
            const uint32_t incl = sb_wave_scan(cnt, lane);
            uint32_t ord = ord0 + incl - cnt;
            for (uint32_t b = ev; b; b &= b - 1u, ord++) {
                const uint32_t bit = (uint32_t)__builtin_ctz(b);
                if (ord < SB_BUDGET) atomicAdd(&s_out[(bit & ~1u) + ((bit & 1u) ? 0u : 1u)], 1u);      // PixelCcClip keeps Under in front of Over
            }
            ord0 += (uint32_t)__shfl((int)incl, 63);
        }
    }
    __syncthreads();
    if (t < 6) dst[37 + t] = s_out[t];
}

// Grid of k_stats_batch: four workgroups per compute unit of the CURRENT device with histograms (38 KiB of LDS each), eight without, never more workgroups than
// there are steps of four units.  Both kernels on `st`; tot / rowcnt zeroed by the caller on the same stream.  0, -1 on a launch error.
int js_launch_stats_batch(hipStream_t st, const int16_t* planes, const JsStatRec* recs, const uint64_t* unit_base, uint32_t nrec, uint64_t total_units, int hist_en,
                          uint32_t* tot, uint32_t* rowcnt, uint32_t* totals_out)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * (hist_en ? 4u : 8u), (total_units + SB_WAVES - 1u) / SB_WAVES);
    const uint64_t units_per_wg = (total_units + want - 1u) / want, grid = (total_units + units_per_wg - 1u) / units_per_wg;
    if (grid > 0x7FFFFFFFull) return -1;
    if (hist_en) hipLaunchKernelGGL(k_stats_batch<true>, dim3((uint32_t)grid), dim3(SB_THREADS), 0, st, planes, recs, unit_base, nrec, total_units, units_per_wg, tot, rowcnt);
    else hipLaunchKernelGGL(k_stats_batch<false>, dim3((uint32_t)grid), dim3(SB_THREADS), 0, st, planes, recs, unit_base, nrec, total_units, units_per_wg, tot, rowcnt);
    hipLaunchKernelGGL(k_stats_order, dim3(nrec), dim3(SB_THREADS), 0, st, planes, recs, tot, rowcnt, totals_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

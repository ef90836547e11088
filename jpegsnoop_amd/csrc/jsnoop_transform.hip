// jsnoop_transform.hip -- k_transform: the DCT blocks of a decoded batch rearranged into the arena and the cumulative DC of a flipped, rotated, transposed,
// cropped or grey picture (geometry, plan and the block map live in jsnoop_transform_check.h, compiled for host and device;
// tests/transform_model.py is the definition).
//
// Work: ONE launch for the whole call.  A unit is a run of up to JS_XF_RUN = 8 consecutive DESTINATION blocks of one entry, done by one wave, eight lanes a
// block; units are numbered through a prefix table over the records (unit_base, nrec + 1 entries) and dealt like k_encode's: a workgroup takes a contiguous
// share, its four waves interleaved, finds the record of its first unit by one search and walks on from there.  What depends on the unit only is wave-uniform.
//   read.   Lane (b, r) maps destination block b of the run to its source block (js_xf_map, the function the host test walks) and reads row r of it: one
//           16-byte load; the eight lanes of a block cover its 128-byte arena row.
//   turn.   Non-transposing ops stay in registers.  Transposing ops (XF_T) write the row into the wave's tile in LDS and read column r back as eight 2-byte
//           reads: a block's tile is 128 bytes at the pitch of XF_BLK_PITCH = 144 that k_encode uses for the same access pair (16-byte rows in, 2-byte columns
//           out; the four blocks of a half-wave start at banks 0, 4, 8, 12 and take four banks each, two lanes a dword: no conflict).
//   sign.   Destination cell [v][u] changes sign where u is odd (JS_XF_NEGU), where v is odd (JS_XF_NEGV), where u + v is odd (both): int16 modulo 2^16, so
//           -32768 stays.  Cell 0 has u = v = 0.  No cell is interpreted.
//   write.  One 16-byte store a lane: a wave-store writes eight whole arena rows, 1 KiB contiguous.  Lane (b, 0) moves the block's cumulative DC.
// Integer arithmetic only; no atomics, no scratch; every global store is a vector store.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_transform_check.h"

#define XF_THREADS 256
#define XF_WAVES   (XF_THREADS / 64)
#define XF_BLK_PITCH 144u
#define XF_WAVE_BYTES (JS_XF_RUN * XF_BLK_PITCH)

typedef uint32_t xf_u32x4 __attribute__((ext_vector_type(4)));
#define XF_GLOBAL __attribute__((address_space(1)))

static_assert(JS_XF_RUN * 8u == 64u, "eight lanes a block, a wave a run");
static_assert(XF_WAVE_BYTES % 16u == 0, "16-byte LDS accesses");

__device__ __forceinline__ void xf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// two int16 in a word, each negated modulo 2^16 where asked
__device__ __forceinline__ uint32_t xf_neg(uint32_t w, bool lo, bool hi)
{
    uint32_t l = w & 0xFFFFu, h = w & 0xFFFF0000u;
    if (lo) l = (0u - l) & 0xFFFFu;
    if (hi) h = 0u - h;
    return l | h;
}

template <bool XF_TRANSPOSING>
__global__ void __launch_bounds__(XF_THREADS) k_transform(const JsXfRec* __restrict__ recs, const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units,
                                                          uint32_t units_per_wg, uint32_t flags, const int16_t* __restrict__ src_coef, const int16_t* __restrict__ src_dccum,
                                                          int16_t* __restrict__ coef, int16_t* __restrict__ dccum)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_mem[XF_TRANSPOSING ? XF_WAVES * XF_WAVE_BYTES : 16];
    const uint32_t lane = threadIdx.x & 63u, bl = lane >> 3, r8 = lane & 7u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* tb = s_mem + (XF_TRANSPOSING ? wave * XF_WAVE_BYTES + bl * XF_BLK_PITCH : 0u);
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t u = u0 + wave;
    if (u >= u1) return;
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u) k = mid; else top = mid; }
    const bool negu = flags & JS_XF_NEGU, negv = flags & JS_XF_NEGV;
    const bool neg_lo = negv && (r8 & 1u), neg_hi = neg_lo != negu;                                 // cells (r8, even u) and (r8, odd u) of the destination row
    while (u < u1) {
        while (u >= unit_base[k + 1]) k++;
        const uint32_t kbeg = unit_base[k], kend = min(u1, unit_base[k + 1]);
        const JsXfRec& r = recs[k];                                           // (wave-uniform: read through the scalar cache, once per entry and share)
        for (; u < kend; u += XF_WAVES) {
            const uint32_t j = (u - kbeg) * JS_XF_RUN + bl; const bool live = j < r.nblk;
            const uint64_t sb = r.src_off + js_xf_map(r, flags, live ? j : 0u), db = r.dst_off + j;
            xf_u32x4 row = *(const XF_GLOBAL xf_u32x4*)(src_coef + sb * 64u + r8 * 8u);             // (a dead lane reads the entry's block 0: inside the source)
            if (XF_TRANSPOSING) {
                *reinterpret_cast<xf_u32x4*>(tb + r8 * 16u) = row;
                xf_wave_sync();
                uint32_t d[8];
                #pragma unroll
                for (int c = 0; c < 8; c++) d[c] = *reinterpret_cast<const uint16_t*>(tb + c * 16 + r8 * 2u);
                row = xf_u32x4{ d[0] | d[1] << 16, d[2] | d[3] << 16, d[4] | d[5] << 16, d[6] | d[7] << 16 };
                xf_wave_sync();                                               // (the next unit's tile writes must not pass these reads)
            }
            row = xf_u32x4{ xf_neg(row.x, neg_lo, neg_hi), xf_neg(row.y, neg_lo, neg_hi), xf_neg(row.z, neg_lo, neg_hi), xf_neg(row.w, neg_lo, neg_hi) };
            if (live) {
                *(XF_GLOBAL xf_u32x4*)(coef + db * 64u + r8 * 8u) = row;
                if (r8 == 0u) *(XF_GLOBAL int16_t*)(dccum + db) = *(const XF_GLOBAL int16_t*)(src_dccum + sb);
            }
        }
    }
}

// Grid: eight workgroups per compute unit of the CURRENT device, never more workgroups than there are steps of four units.  0, -1 on a launch error.
int js_launch_transform(hipStream_t st, const JsXfRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units, uint32_t flags,
                        const int16_t* src_coef, const int16_t* src_dccum, int16_t* coef, int16_t* dccum)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 8u, ((uint64_t)total_units + XF_WAVES - 1u) / XF_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (flags & JS_XF_T) hipLaunchKernelGGL(k_transform<true>, dim3(grid), dim3(XF_THREADS), 0, st, recs, unit_base, nrec, total_units, units_per_wg, flags, src_coef, src_dccum, coef, dccum);
    else hipLaunchKernelGGL(k_transform<false>, dim3(grid), dim3(XF_THREADS), 0, st, recs, unit_base, nrec, total_units, units_per_wg, flags, src_coef, src_dccum, coef, dccum);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// jsnoop_coef.hip -- k_pack_coefs: the coefficient arena of a decoded batch into caller-owned device memory, one tensor per component.
//
// The arena is [blocks][64] int16 in natural order and decode order (MCU after MCU, components interleaved), slot 0 = the DC difference; the cumulative DC
// of a block is in a second arena (dccum).  A destination is one component of one image: its blocks in raster order of the component's own block grid
// (bw x bh), the cumulative DC in natural index 0, block-major [bh][bw][64] or frequency-major [64][bh][bw], int16 or float, natural or zig-zag order.
// Pure data movement: no arithmetic on a value except the exact int16 -> float conversion.
//
// Work: ONE launch for the whole list.  A unit is a run of up to JS_COEF_TILE = 64 blocks, consecutive in bx, of one row of a block grid, done by one
// wave: eight lanes a block, a lane reads 16 bytes (eight coefficients) of each of eight blocks -- eight loads in flight before the first store --
// and the lane that owns natural index 0 swaps in the dccum value.  Units are numbered through a prefix table over the records (unit_base, nrec + 1
// entries) and dealt like k_pack_rgb's: a workgroup takes a contiguous share, its four waves interleaved, finds the record of its first unit by one
// search and walks on from there.  Everything that depends on the unit only is wave-uniform and lives in scalar registers.
//
// Forms.
//   BLOCKS / NATURAL: registers to memory.  A lane stores the 16 bytes it read (int16) or two 16-byte vectors (float); a wave-store covers eight whole
//     output blocks, contiguous along bx (1 KiB / 2 KiB).  No LDS.
//   everything else goes through a wave-private LDS tile of 64 blocks x 128 bytes.  A block's eight 16-byte chunks are stored permuted: chunk c of block b
//     lies at chunk c ^ (b >> 3).  The 16-byte writes of a block's eight lanes then still cover its 128 bytes exactly once (ds_write_b128: groups of
//     eight lanes, 32 banks), and the transposed reads below touch 16 different banks per 32-lane group.
//   BLOCKS / ZIGZAG: the lane that owns positions 8 s .. 8 s + 7 of a block gathers its eight natural indices from the block's row by 2-byte LDS reads
//     and stores as above.
//   FREQ: a real transposition.  Lane (f, j) = (lane >> 3, lane & 7) gathers, for position 8 g + f (g = 0..7), the values of blocks 8 j .. 8 j + 7 of the
//     tile -- eight 2-byte LDS reads at a stride of one block; in natural order the 32 lanes of a group read 16 dwords in 16 banks -- and stores them as ONE
//     16-byte vector (int16; two for float): a wave-store writes, for each of eight frequencies, 128 (256) contiguous bytes of that frequency's plane.
//     The tail of a row (fewer than 64 blocks left, or a row shorter than a tile) takes the narrow path for its last, incomplete group of eight blocks:
//     single 2- or 4-byte stores.  Zig-zag order only changes which natural index a lane gathers; its reads can conflict.
// Destinations may start at any multiple of the element size: the vector stores rely on the unaligned global stores the library probes for at start-up
// (k_unaligned_probe), as k_pack_rgb's do.  Only addressed elements are written.  No atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"

#define CF_THREADS 256
#define CF_WAVES   (CF_THREADS / 64)
#define CF_TILE_BYTES (JS_COEF_TILE * 128u)          /* LDS of one wave */

typedef uint32_t cf_u32x4 __attribute__((ext_vector_type(4)));
typedef float    cf_f32x4 __attribute__((ext_vector_type(4)));
#define CF_GLOBAL __attribute__((address_space(1)))
typedef cf_u32x4 cf_u32x4_a2 __attribute__((aligned(2)));
typedef cf_f32x4 cf_f32x4_a4 __attribute__((aligned(4)));

__constant__ uint8_t c_cf_zigzag[64] = JS_ZIGZAG_NATURAL;

// eight int16 (w: four dwords, low half first) to o[0 .. 7] of the destination's element type
template <int DTYPE>
__device__ __forceinline__ void cf_store8(CF_GLOBAL uint8_t* o, cf_u32x4 w)
{
    if (DTYPE == JSNOOP_COEF_I16) *reinterpret_cast<CF_GLOBAL cf_u32x4_a2*>(o) = w;
    else {
        const cf_f32x4 a = { (float)(int16_t)w.x, (float)((int32_t)w.x >> 16), (float)(int16_t)w.y, (float)((int32_t)w.y >> 16) },
                       b = { (float)(int16_t)w.z, (float)((int32_t)w.z >> 16), (float)(int16_t)w.w, (float)((int32_t)w.w >> 16) };
        CF_GLOBAL cf_f32x4_a4* o4 = reinterpret_cast<CF_GLOBAL cf_f32x4_a4*>(o); o4[0] = a; o4[1] = b;
    }
}
template <int DTYPE>
__device__ __forceinline__ void cf_store1(CF_GLOBAL uint8_t* o, uint32_t v16)
{
    if (DTYPE == JSNOOP_COEF_I16) *reinterpret_cast<CF_GLOBAL uint16_t*>(o) = (uint16_t)v16;
    else *reinterpret_cast<CF_GLOBAL float*>(o) = (float)(int16_t)v16;
}

template <int LAYOUT, int DTYPE, int ORDER>
__global__ void __launch_bounds__(CF_THREADS) k_pack_coefs(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsCoefRec* __restrict__ recs,
                                                           const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units, uint32_t units_per_wg)
{
    constexpr bool DIRECT = LAYOUT == JSNOOP_COEF_BLOCKS && ORDER == JSNOOP_COEF_NATURAL;
    constexpr uint32_t ELEM = DTYPE == JSNOOP_COEF_F32 ? 4u : 2u;
    extern __shared__ __attribute__((aligned(16))) uint8_t s_tiles[];            // CF_WAVES tiles (none in the DIRECT form)
    const uint32_t lane = threadIdx.x & 63u, hi = lane >> 3, lo = lane & 7u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* tile = s_tiles + (DIRECT ? 0u : wave * CF_TILE_BYTES);
    // this workgroup's share of the units: [u0, u1)
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t u = u0 + wave;
    if (u >= u1) return;
    // which natural indices this lane gathers from the tile: byte offset inside the 16-byte chunk, and the chunk
    uint32_t g_off[8], g_chunk[8];
    if (!DIRECT) {
        #pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t pos = LAYOUT == JSNOOP_COEF_BLOCKS ? lo * 8u + e : e * 8u + hi;         // BLOCKS: positions 8 lo .. 8 lo + 7 of a block; FREQ: position 8 e + hi, e = the pass
            const uint32_t nat = ORDER == JSNOOP_COEF_ZIGZAG ? (uint32_t)c_cf_zigzag[pos] : pos;
            g_off[e] = (nat & 7u) * 2u; g_chunk[e] = nat >> 3;
        }
    }
    // the record of the first unit: the last k with unit_base[k] <= u (unit_base[0] = 0, unit_base[nrec] = total_units > u)
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u) k = mid; else top = mid; }
    uint32_t kbeg = 0, kend = 0; bool fresh = true;
    uint32_t bw = 0, sh = 1, sv = 1, first = 0, bpm = 1, mcu_xmax = 0, tiles = 1; uint64_t row_pitch = 0, plane_pitch = 0, coef_off = 0; CF_GLOBAL uint8_t* dst = nullptr;
    for (; u < u1; u += CF_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            const JsCoefRec r = recs[k];
            bw = r.bw; sh = r.sh; sv = r.sv; first = r.first; bpm = r.bpm; mcu_xmax = r.mcu_xmax; tiles = r.tiles; coef_off = r.coef_off;
            dst = reinterpret_cast<CF_GLOBAL uint8_t*>(r.ptr); row_pitch = r.row_pitch; plane_pitch = r.plane_pitch;
        }
        const uint32_t lu = u - kbeg, by = lu / tiles, bx0 = (lu - by * tiles) * JS_COEF_TILE, nblk = min(JS_COEF_TILE, bw - bx0);
        const uint32_t my = by / sv, vy = by - my * sv;
        const uint64_t row_blk = coef_off + (uint64_t)my * mcu_xmax * bpm + first + vy * sh;      // arena block of (MCU column 0, ch 0) of this block row
        CF_GLOBAL uint8_t* row = dst + (size_t)by * row_pitch;

        // ---- load: pass p takes blocks 8 p .. 8 p + 7 of the run, lane (hi, lo) chunk lo of block 8 p + hi
        cf_u32x4 v[8];
        #pragma unroll
        for (int p = 0; p < 8; p++) {
            const uint32_t b = p * 8u + hi, bx = bx0 + b;
            v[p] = cf_u32x4{ 0u, 0u, 0u, 0u };
            if (b < nblk) {
                const uint32_t mx = sh == 1u ? bx : (sh == 2u ? bx >> 1 : (sh == 4u ? bx >> 2 : bx / 3u)), hx = bx - mx * sh;
                const uint64_t blk = row_blk + (uint64_t)mx * bpm + hx;
                v[p] = *reinterpret_cast<const cf_u32x4*>(coef + blk * 64u + lo * 8u);
                if (lo == 0u) v[p].x = (v[p].x & 0xFFFF0000u) | (uint32_t)(uint16_t)dccum[blk];
            }
        }
        if (DIRECT) {
            #pragma unroll
            for (int p = 0; p < 8; p++) {
                const uint32_t b = p * 8u + hi;
                if (b < nblk) cf_store8<DTYPE>(row + ((size_t)(bx0 + b) * 64u + lo * 8u) * ELEM, v[p]);
            }
            continue;
        }
        // ---- stage: chunk lo of block b at chunk lo ^ (b >> 3) of the block's row (blocks past the run: zeros, never stored)
        #pragma unroll
        for (int p = 0; p < 8; p++)
            *reinterpret_cast<cf_u32x4*>(tile + (p * 8u + hi) * 128u + ((lo ^ (uint32_t)p) << 4)) = v[p];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (LAYOUT == JSNOOP_COEF_BLOCKS) {
            // lane (hi, lo): positions 8 lo .. 8 lo + 7 of block 8 p + hi
            #pragma unroll
            for (int p = 0; p < 8; p++) {
                const uint32_t b = p * 8u + hi;
                const uint8_t* src = tile + b * 128u;
                uint32_t h[8];
                #pragma unroll
                for (int e = 0; e < 8; e++) h[e] = *reinterpret_cast<const uint16_t*>(src + ((g_chunk[e] ^ (uint32_t)p) << 4) + g_off[e]);
                const cf_u32x4 w = { h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16) };
                if (b < nblk) cf_store8<DTYPE>(row + ((size_t)(bx0 + b) * 64u + lo * 8u) * ELEM, w);
            }
        } else {
            // lane (hi, lo): position 8 g + hi, blocks 8 lo .. 8 lo + 7 of the run
            const uint32_t b0 = lo * 8u, m = nblk > b0 ? min(8u, nblk - b0) : 0u;
            const uint8_t* src = tile + b0 * 128u;
            #pragma unroll
            for (int g = 0; g < 8; g++) {
                const uint32_t a = ((g_chunk[g] ^ lo) << 4) + g_off[g];
                uint32_t h[8];
                #pragma unroll
                for (int i = 0; i < 8; i++) h[i] = *reinterpret_cast<const uint16_t*>(src + i * 128u + a);
                CF_GLOBAL uint8_t* o = row + (size_t)(g * 8u + hi) * plane_pitch + (size_t)(bx0 + b0) * ELEM;
                if (m == 8u) {
                    const cf_u32x4 w = { h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16) };
                    cf_store8<DTYPE>(o, w);
                } else {
                    #pragma unroll
                    for (int i = 0; i < 7; i++) if ((uint32_t)i < m) cf_store1<DTYPE>(o + i * ELEM, h[i]);
                }
            }
        }
        // (the next unit's staging writes must not pass these reads)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Grid: eight workgroups per compute unit of the CURRENT device for the register form, five for the forms with an LDS tile (32 KiB per workgroup of the
// 160 KiB), never more workgroups than there are steps of four units.  0, -1 on a launch error or an unknown form.
template <int LAYOUT, int DTYPE, int ORDER>
static void cf_launch(hipStream_t st, uint32_t grid, const int16_t* coef, const int16_t* dccum, const JsCoefRec* recs, const uint32_t* unit_base, uint32_t nrec,
                      uint32_t total_units, uint32_t units_per_wg)
{
    constexpr bool direct = LAYOUT == JSNOOP_COEF_BLOCKS && ORDER == JSNOOP_COEF_NATURAL;
    hipLaunchKernelGGL((k_pack_coefs<LAYOUT, DTYPE, ORDER>), dim3(grid), dim3(CF_THREADS), direct ? 0u : CF_WAVES * CF_TILE_BYTES, st,
                       coef, dccum, recs, unit_base, nrec, total_units, units_per_wg);
}
int js_launch_pack_coefs(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsCoefRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                         int layout, int dtype, int order)
{
    if (!nrec || !total_units) return 0;
    if ((layout | 1) != 1 || (dtype | 1) != 1 || (order | 1) != 1) return -1;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const bool direct = layout == JSNOOP_COEF_BLOCKS && order == JSNOOP_COEF_NATURAL;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * (direct ? 8u : 5u), ((uint64_t)total_units + CF_WAVES - 1u) / CF_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    switch (layout * 4 + dtype * 2 + order) {
    case 0: cf_launch<0, 0, 0>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 1: cf_launch<0, 0, 1>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 2: cf_launch<0, 1, 0>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 3: cf_launch<0, 1, 1>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 4: cf_launch<1, 0, 0>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 5: cf_launch<1, 0, 1>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    case 6: cf_launch<1, 1, 0>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    default: cf_launch<1, 1, 1>(st, grid, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// jsnoop_render.hip -- k_render_ijg: the coefficient arena of a decoded batch rendered as libjpeg's pixels into caller-owned device memory (DESIGN.md section
// 4.21; the arithmetic is libjpeg's integer path and lives in jsnoop_render_check.h, compiled for host and device; tests/ijg_model.py is the definition).
//
// Work: ONE launch for the whole list.  A unit is a run of up to JS_REN_RUN = 8 consecutive MCUs of one MCU row of one image, done by one wave; units are
// numbered through a prefix table over the records (unit_base, nrec + 1 entries) and dealt like k_encode's: a workgroup takes a contiguous share, its four
// waves interleaved, finds the record of its first unit by one search and walks on from there.  What depends on the unit only is wave-uniform.  Waves share
// nothing: what the chroma filter reads from outside the unit (one chroma column left and right, for 4:2:0 one chroma row above and below) the wave
// transforms itself from the arena -- the halo jobs of js_ren_job.
//
// A unit, in two steps, both through the wave's own LDS (JS_REN_WAVE_BYTES):
//   1. inverse DCT, eight jobs a pass, eight lanes a job.  Lane (b, r) loads row r of the job's block as one 16-byte vector (index 0 from dccum), widens it
//      and writes it into the transpose tile; lane (b, c) reads column c (eight dword reads), runs pass 1 on eight values in registers and writes them back
//      over the cells it read; lane (b, r) reads row r of the workspace (two 16-byte reads), runs pass 2, saturates and writes the samples the job keeps into
//      the byte planes: all eight (an own block: one 8-byte write), or one row / one column / one corner sample of a halo block.  A block's tile is 64
//      dwords at a pitch of JS_REN_BLK_PITCH = 72: at one row index the column accesses of the eight blocks of a pass fall on dwords 72 b + 8 k + c, that is
//      banks 8 b + c (mod 64) -- 64 lanes, 64 different dwords, no two on one bank in either half of the wave; at the dense pitch of 64 all eight blocks
//      would meet on the same eight banks.  The 16-byte row accesses touch dwords 72 b + 8 r + (0..3 | 4..7): within a block rows r and r + 4 share four
//      banks, a two-way conflict that is left in (two of the ten LDS instructions of a pass).
//   2. upsampling, colour and store, lane = four consecutive pixels of one row, two rows a step (lanes 0..31 / 32..63).  Chroma neighbours are looked up
//      through js_ren_clamp_col / _row: the clamp of the contract is applied to the index, so a halo cell is read only where a job wrote it.  Stores are
//      k_pack_rgb's forms: four pixels are 12 contiguous bytes (HWC uint8), one dword per plane (CHW uint8), three or one 16-byte vectors (float); a uint8 row
//      may start at any byte (the unaligned vector stores k_unaligned_probe verifies); the tail of a row is single byte / float stores.
// Integer arithmetic only (the float forms: one multiply, one add, separately rounded); no atomics, no scratch; every global store is a vector store.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_render_check.h"

#define RN_THREADS 256
#define RN_WAVES   (RN_THREADS / 64)

typedef uint32_t rn_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rn_u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t rn_u32x2 __attribute__((ext_vector_type(2)));
typedef float    rn_f32x4 __attribute__((ext_vector_type(4)));
#define RN_GLOBAL __attribute__((address_space(1)))
typedef rn_u32x3 rn_u32x3_a1 __attribute__((aligned(1)));
typedef uint32_t rn_u32_a1   __attribute__((aligned(1)));
typedef rn_f32x4 rn_f32x4_a4 __attribute__((aligned(4)));

static_assert(JS_REN_WAVE_BYTES % 16u == 0 && JS_REN_OFF_TILE % 16u == 0 && JS_REN_OFF_C % 8u == 0 && JS_REN_C_BYTES % 8u == 0 && JS_REN_C_PITCH % 8u == 0, "aligned LDS accesses");
static_assert(JS_REN_RUN * 16u == JS_REN_Y_PITCH && JS_REN_RUN * 8u + 9u <= JS_REN_C_PITCH, "a unit fits its planes");

__device__ __forceinline__ void rn_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n <= 4 pixels from x on; byte c of v[j] = output channel c of pixel j.  k_pack_rgb's store forms.
template <int LAYOUT, int DTYPE>
__device__ __forceinline__ void rn_store(RN_GLOBAL uint8_t* row /* ptr + y * row_pitch */, uint64_t plane_pitch, uint32_t x, uint32_t n, const uint32_t v[4], const JsPackArgs& a)
{
    if (n == 0u) return;
    if (DTYPE == JSNOOP_PACK_U8) {
        if (LAYOUT == JSNOOP_PACK_HWC) {
            RN_GLOBAL uint8_t* o = row + (size_t)x * 3;
            if (n == 4u) {
                rn_u32x3 w;
                w.x = (v[0] & 0xFFFFFFu) | (v[1] << 24);
                w.y = ((v[1] >> 8) & 0xFFFFu) | (v[2] << 16);
                w.z = ((v[2] >> 16) & 0xFFu) | (v[3] << 8);
                // (must stay ONE 12-byte store, as in k_pack_rgb: the guard bands of tests/test_gpu_pack_ijg.py catch a stray dword)
                *reinterpret_cast<RN_GLOBAL rn_u32x3_a1*>(o) = w;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = (uint8_t)v[j]; o[3 * j + 1] = (uint8_t)(v[j] >> 8); o[3 * j + 2] = (uint8_t)(v[j] >> 16); }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                RN_GLOBAL uint8_t* o = row + (size_t)c * plane_pitch + x;
                if (n == 4u) {
                    *reinterpret_cast<RN_GLOBAL rn_u32_a1*>(o) = ((v[0] >> (8 * c)) & 0xFFu) | (((v[1] >> (8 * c)) & 0xFFu) << 8) |
                                                       (((v[2] >> (8 * c)) & 0xFFu) << 16) | (((v[3] >> (8 * c)) & 0xFFu) << 24);
                } else {
                    #pragma unroll
                    for (int j = 0; j < 3; j++) if ((uint32_t)j < n) o[j] = (uint8_t)(v[j] >> (8 * c));
                }
            }
        }
    } else {
        // out = (float)v * scale[c] + bias[c]: one rounded multiply, one rounded add, never an FMA
        float f[4][3];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            #pragma unroll
            for (int c = 0; c < 3; c++) f[j][c] = __fadd_rn(__fmul_rn((float)((v[j] >> (8 * c)) & 0xFFu), a.scale[c]), a.bias[c]);
        }
        if (LAYOUT == JSNOOP_PACK_HWC) {
            RN_GLOBAL float* o = reinterpret_cast<RN_GLOBAL float*>(row + (size_t)x * 12);
            if (n == 4u) {
                rn_f32x4 w0 = { f[0][0], f[0][1], f[0][2], f[1][0] }, w1 = { f[1][1], f[1][2], f[2][0], f[2][1] }, w2 = { f[2][2], f[3][0], f[3][1], f[3][2] };
                RN_GLOBAL rn_f32x4_a4* o4 = reinterpret_cast<RN_GLOBAL rn_f32x4_a4*>(o); o4[0] = w0; o4[1] = w1; o4[2] = w2;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = f[j][0]; o[3 * j + 1] = f[j][1]; o[3 * j + 2] = f[j][2]; }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                RN_GLOBAL float* o = reinterpret_cast<RN_GLOBAL float*>(row + (size_t)c * plane_pitch + (size_t)x * 4);
                if (n == 4u) { rn_f32x4 w = { f[0][c], f[1][c], f[2][c], f[3][c] }; *reinterpret_cast<RN_GLOBAL rn_f32x4_a4*>(o) = w; }
                else {
                    #pragma unroll
                    for (int j = 0; j < 3; j++) if ((uint32_t)j < n) o[j] = f[j][c];
                }
            }
        }
    }
}

template <int LAYOUT, int DTYPE>
__global__ void __launch_bounds__(RN_THREADS) k_render_ijg(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsRenRec* __restrict__ recs,
                                                           const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, JsPackArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_mem[RN_WAVES * JS_REN_WAVE_BYTES];
    const uint32_t lane = threadIdx.x & 63u, bl = lane >> 3, r8 = lane & 7u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* mem = s_mem + wave * JS_REN_WAVE_BYTES;
    int32_t* tb = reinterpret_cast<int32_t*>(mem + JS_REN_OFF_TILE) + bl * JS_REN_BLK_PITCH;
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t u = u0 + wave;
    if (u >= u1) return;
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u) k = mid; else top = mid; }
    uint32_t kbeg = 0, kend = 0; bool fresh = true;
    JsRenRec r;
    for (; u < u1; u += RN_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            r = recs[k];
        }
        const uint32_t lu = u - kbeg, my = lu / r.runs, m0 = (lu - my * r.runs) * JS_REN_RUN, nm = min(JS_REN_RUN, r.mcu_xmax - m0);
        const uint32_t mcu_w = 8u * r.H, mcu_h = 8u * r.V, x0 = m0 * mcu_w, y0 = my * mcu_h;

        // ---- 1. inverse DCT, eight jobs a pass
        const uint32_t njobs = js_ren_jobs(r, nm);
        for (uint32_t j0 = 0; j0 < njobs; j0 += 8u) {
            const JsRenJob job = js_ren_job(r, my, m0, nm, j0 + bl, r8);
            int32_t d[8];
            #pragma unroll
            for (int i = 0; i < 8; i++) d[i] = 0;
            if (job.exists) {
                const uint64_t blk = r.coef_off + job.blk;
                const rn_u32x4 raw = *reinterpret_cast<const rn_u32x4*>(coef + blk * 64u + r8 * 8u);
                d[0] = (int16_t)raw.x; d[1] = (int32_t)raw.x >> 16; d[2] = (int16_t)raw.y; d[3] = (int32_t)raw.y >> 16;
                d[4] = (int16_t)raw.z; d[5] = (int32_t)raw.z >> 16; d[6] = (int16_t)raw.w; d[7] = (int32_t)raw.w >> 16;
                if (r8 == 0u) d[0] = dccum[blk];
            }
            *reinterpret_cast<rn_u32x4*>(tb + r8 * 8u) = rn_u32x4{ (uint32_t)d[0], (uint32_t)d[1], (uint32_t)d[2], (uint32_t)d[3] };
            *reinterpret_cast<rn_u32x4*>(tb + r8 * 8u + 4u) = rn_u32x4{ (uint32_t)d[4], (uint32_t)d[5], (uint32_t)d[6], (uint32_t)d[7] };
            rn_wave_sync();
            #pragma unroll
            for (int v = 0; v < 8; v++) d[v] = tb[v * 8 + r8];
            js_ren_idct_step<11>(d);
            #pragma unroll
            for (int v = 0; v < 8; v++) tb[v * 8 + r8] = d[v];
            rn_wave_sync();
            const rn_u32x4 lo = *reinterpret_cast<const rn_u32x4*>(tb + r8 * 8u), hi = *reinterpret_cast<const rn_u32x4*>(tb + r8 * 8u + 4u);
            d[0] = (int32_t)lo.x; d[1] = (int32_t)lo.y; d[2] = (int32_t)lo.z; d[3] = (int32_t)lo.w; d[4] = (int32_t)hi.x; d[5] = (int32_t)hi.y; d[6] = (int32_t)hi.z; d[7] = (int32_t)hi.w;
            js_ren_idct_step<18>(d);
            uint32_t smp[8];
            #pragma unroll
            for (int i = 0; i < 8; i++) smp[i] = js_ren_sample(d[i]);
            if (job.mask == 0xFFu) {
                *reinterpret_cast<rn_u32x2*>(mem + job.dst0) = rn_u32x2{ smp[0] | (smp[1] << 8) | (smp[2] << 16) | (smp[3] << 24), smp[4] | (smp[5] << 8) | (smp[6] << 16) | (smp[7] << 24) };
            } else if (job.mask == 0x80u) mem[job.dst0 + 7u] = (uint8_t)smp[7];
            else if (job.mask == 0x01u) mem[job.dst0] = (uint8_t)smp[0];
            rn_wave_sync();                                               // (the next pass's tile writes must not pass these reads; the planes are complete behind the last)
        }

        // ---- 2. upsampling, colour, store: lane = four pixels, two rows a step
        const uint32_t wpix = min(nm * mcu_w, r.dim_x - x0), hpix = min(mcu_h, r.dim_y - y0), lx = (lane & 31u) * 4u;
        const uint32_t dw = (r.dim_x + r.H - 1u) / r.H, dh = (r.dim_y + r.V - 1u) / r.V;
        RN_GLOBAL uint8_t* dst = reinterpret_cast<RN_GLOBAL uint8_t*>(r.ptr);
        if (lx < wpix) {
            const uint32_t n = min(4u, wpix - lx);
            for (uint32_t ly = lane >> 5; ly < hpix; ly += 2u) {
                const uint32_t y4 = *reinterpret_cast<const uint32_t*>(mem + ly * JS_REN_Y_PITCH + lx);
                uint32_t v[4];
                if (r.ncomp == 1u) {
                    #pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = ((y4 >> (8 * j)) & 0xFFu) * 0x010101u;
                } else {
                    uint32_t cb[4], cr[4];
                    const uint8_t* pb = mem + JS_REN_OFF_C; const uint8_t* pr = pb + JS_REN_C_BYTES;
                    if (r.H == 1u) {
                        const uint32_t at = (1u + ly) * JS_REN_C_PITCH + 8u + lx;
                        const uint32_t b4 = *reinterpret_cast<const uint32_t*>(pb + at), r4 = *reinterpret_cast<const uint32_t*>(pr + at);
                        #pragma unroll
                        for (int j = 0; j < 4; j++) { cb[j] = (b4 >> (8 * j)) & 0xFFu; cr[j] = (r4 >> (8 * j)) & 0xFFu; }
                    } else {
                        js_ren_chroma4(pb, r.V, y0 + ly, (x0 + lx) >> 1, dw, dh, my, m0, cb);
                        js_ren_chroma4(pr, r.V, y0 + ly, (x0 + lx) >> 1, dw, dh, my, m0, cr);
                    }
                    #pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t rgb = js_ren_rgb((y4 >> (8 * j)) & 0xFFu, cb[j], cr[j]);
                        v[j] = a.bgr ? ((rgb >> 16) & 0xFFu) | (rgb & 0xFF00u) | ((rgb & 0xFFu) << 16) : rgb;
                    }
                }
                rn_store<LAYOUT, DTYPE>(dst + (size_t)(y0 + ly) * r.row_pitch, r.plane_pitch, x0 + lx, n, v, a);
            }
        }
        rn_wave_sync();                                                   // (the next unit's plane writes must not pass these reads)
    }
}

// Grid: six workgroups per compute unit of the CURRENT device (24 KiB of LDS each), never more workgroups than there are steps of four units.
// 0, -1 on a launch error or an unknown layout / dtype.
int js_launch_render_ijg(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsRenRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                         int layout, int dtype, const JsPackArgs& a)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 6u, ((uint64_t)total_units + RN_WAVES - 1u) / RN_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_render_ijg<JSNOOP_PACK_HWC, JSNOOP_PACK_U8>), dim3(grid), dim3(RN_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_render_ijg<JSNOOP_PACK_CHW, JSNOOP_PACK_U8>), dim3(grid), dim3(RN_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_render_ijg<JSNOOP_PACK_HWC, JSNOOP_PACK_F32>), dim3(grid), dim3(RN_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_render_ijg<JSNOOP_PACK_CHW, JSNOOP_PACK_F32>), dim3(grid), dim3(RN_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

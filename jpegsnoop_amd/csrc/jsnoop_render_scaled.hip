// jsnoop_render_scaled.hip -- k_render_ijg_scaled: the coefficient arena of a decoded batch rendered as libjpeg's REDUCED-SIZE pixels (1/2, 1/4, 1/8) into
// caller-owned device memory (the arithmetic and every stage of a unit's walk live in jsnoop_render_scaled_check.h, compiled for host and
// device; tests/ijg_scaled_model.py is the definition).
//
// Work: ONE launch for the whole list.  With m = 8 / denom an MCU gives H m x V m pixels; a unit is a run of up to 64 / (H m) consecutive MCUs of one MCU row of one
// image -- 64 pixels wide, V m rows high -- done by one wave; units are numbered through a prefix table over the records and dealt like k_render_ijg's: a
// workgroup takes a contiguous share, its four waves interleaved, finds the record of its first unit by one search and walks on from there.  The scale comes from
// the record and is wave-uniform (one switch per phase picks the transform; a call of mixed records would be served by the same code, and four store forms stay four
// kernels, not twelve).  Waves share nothing: the one thing read from outside the unit -- the chroma column left and right of a 4:2:2 unit at denom 2 and 4 -- the
// wave transforms itself (the halo jobs of js_rs_job).
//
// A unit, in two phases of transforms (luma at ny, then Cb and Cr at nc) and one of pixels, all through the wave's own LDS (JS_RS_WAVE_BYTES):
//   n = 1: lane = block, dccum alone is read.
//   n = 2, 4, 8: groups of 64 / n jobs.  A group is loaded and column-transformed in 8 / n sub-rounds of eight jobs, eight lanes a job (js_rs_load: lane (b, r)
//      fetches row r as one 16-byte vector if the transform reads that row; js_rs_pass1: lane (b, c) transforms column c if the transform reads that column) into
//      a workspace of 64 rows; then ONE pass 2 for the whole group, lane L = workspace row L (js_rs_pass2) -- every lane of the wave has a row at every n.
//   pixels: lane = four consecutive pixels of one row, four rows a step (js_rs_pixels); stores are k_pack_rgb's forms as k_render_ijg has them.
// Integer arithmetic only (the float forms: one multiply, one add, separately rounded); no atomics, no scratch; every global store is a vector store.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_render_scaled_check.h"

#define RS_THREADS 256
#define RS_WAVES   (RS_THREADS / 64)

typedef uint32_t rs_u32x3 __attribute__((ext_vector_type(3)));
typedef float    rs_f32x4 __attribute__((ext_vector_type(4)));
#define RS_GLOBAL __attribute__((address_space(1)))
typedef rs_u32x3 rs_u32x3_a1 __attribute__((aligned(1)));
typedef uint32_t rs_u32_a1   __attribute__((aligned(1)));
typedef rs_f32x4 rs_f32x4_a4 __attribute__((aligned(4)));

static_assert(JS_RS_WAVE_BYTES % 16u == 0 && JS_RS_OFF_TILE % 16u == 0 && JS_RS_OFF_WS % 16u == 0 && JS_RS_PLANE_BYTES % 8u == 0 && JS_RS_PITCH % 8u == 0, "aligned LDS accesses");
static_assert(8u + 64u + 1u <= JS_RS_PITCH && sizeof(JsRsRec) == 96, "a unit fits its planes");

__device__ __forceinline__ void rs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n <= 4 pixels from x on; byte c of v[j] = output channel c of pixel j.  k_pack_rgb's store forms, as k_render_ijg has them.
template <int LAYOUT, int DTYPE>
__device__ __forceinline__ void rs_store(RS_GLOBAL uint8_t* row /* ptr + y * row_pitch */, uint64_t plane_pitch, uint32_t x, uint32_t n, const uint32_t v[4], const JsPackArgs& a)
{
    if (n == 0u) return;
    if (DTYPE == JSNOOP_PACK_U8) {
        if (LAYOUT == JSNOOP_PACK_HWC) {
            RS_GLOBAL uint8_t* o = row + (size_t)x * 3;
            if (n == 4u) {
                rs_u32x3 w;
                w.x = (v[0] & 0xFFFFFFu) | (v[1] << 24);
                w.y = ((v[1] >> 8) & 0xFFFFu) | (v[2] << 16);
                w.z = ((v[2] >> 16) & 0xFFu) | (v[3] << 8);
                // (must stay ONE 12-byte store: the guard bands of tests/test_gpu_pack_ijg_scaled.py catch a stray dword)
                *reinterpret_cast<RS_GLOBAL rs_u32x3_a1*>(o) = w;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = (uint8_t)v[j]; o[3 * j + 1] = (uint8_t)(v[j] >> 8); o[3 * j + 2] = (uint8_t)(v[j] >> 16); }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                RS_GLOBAL uint8_t* o = row + (size_t)c * plane_pitch + x;
                if (n == 4u) {
                    *reinterpret_cast<RS_GLOBAL rs_u32_a1*>(o) = ((v[0] >> (8 * c)) & 0xFFu) | (((v[1] >> (8 * c)) & 0xFFu) << 8) |
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
            RS_GLOBAL float* o = reinterpret_cast<RS_GLOBAL float*>(row + (size_t)x * 12);
            if (n == 4u) {
                rs_f32x4 w0 = { f[0][0], f[0][1], f[0][2], f[1][0] }, w1 = { f[1][1], f[1][2], f[2][0], f[2][1] }, w2 = { f[2][2], f[3][0], f[3][1], f[3][2] };
                RS_GLOBAL rs_f32x4_a4* o4 = reinterpret_cast<RS_GLOBAL rs_f32x4_a4*>(o); o4[0] = w0; o4[1] = w1; o4[2] = w2;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = f[j][0]; o[3 * j + 1] = f[j][1]; o[3 * j + 2] = f[j][2]; }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                RS_GLOBAL float* o = reinterpret_cast<RS_GLOBAL float*>(row + (size_t)c * plane_pitch + (size_t)x * 4);
                if (n == 4u) { rs_f32x4 w = { f[0][c], f[1][c], f[2][c], f[3][c] }; *reinterpret_cast<RS_GLOBAL rs_f32x4_a4*>(o) = w; }
                else {
                    #pragma unroll
                    for (int j = 0; j < 3; j++) if ((uint32_t)j < n) o[j] = f[j][c];
                }
            }
        }
    }
}

// one phase of a unit at transform size N >= 2: groups of 64 / N jobs, 8 / N sub-rounds of loads and column steps each, then one row step for the whole wave
template <int N>
__device__ __forceinline__ void rs_phase(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t njobs, uint32_t lane, const int16_t* __restrict__ coef,
                                         const int16_t* __restrict__ dccum, uint8_t* mem)
{
    for (uint32_t g0 = 0; g0 < njobs; g0 += 64u / N) {
        for (uint32_t q = 0; q < 8u / N && g0 + q * 8u < njobs; q++) {
            js_rs_load<N>(r, u, phase, g0 + q * 8u, lane, coef, dccum, mem);
            rs_wave_sync();
            js_rs_pass1<N>(r, u, phase, g0 + q * 8u, q, lane, mem);
            rs_wave_sync();                                               // (the next sub-round's tile writes must not pass these reads)
        }
        js_rs_pass2<N>(r, u, phase, g0, lane, mem);
        rs_wave_sync();                                                   // (the next group's workspace writes must not pass these reads)
    }
}

template <int LAYOUT, int DTYPE>
__global__ void __launch_bounds__(RS_THREADS) k_render_ijg_scaled(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsRsRec* __restrict__ recs,
                                                                  const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, JsPackArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_mem[RS_WAVES * JS_RS_WAVE_BYTES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* mem = s_mem + wave * JS_RS_WAVE_BYTES;
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t un = u0 + wave;
    if (un >= u1) return;
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= un) k = mid; else top = mid; }
    uint32_t kbeg = 0, kend = 0; bool fresh = true;
    JsRsRec r;
    for (; un < u1; un += RS_WAVES) {
        if (fresh || un >= kend) {
            while (un >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            r = recs[k];
        }
        const uint32_t lu = un - kbeg;
        JsRsUnit u; u.my = lu / r.runs; u.m0 = (lu - u.my * r.runs) * r.run; u.nm = min(r.run, r.mcu_xmax - u.m0);

        // ---- transforms: luma, then chroma
        for (uint32_t phase = 0; phase < 2u; phase++) {
            const uint32_t njobs = js_rs_jobs(r, u.nm, phase), n = js_rs_n(r, phase);
            if (n == 8u) rs_phase<8>(r, u, phase, njobs, lane, coef, dccum, mem);
            else if (n == 4u) rs_phase<4>(r, u, phase, njobs, lane, coef, dccum, mem);
            else if (n == 2u) rs_phase<2>(r, u, phase, njobs, lane, coef, dccum, mem);
            else for (uint32_t jb = lane; jb < njobs; jb += 64u) js_rs_dc_job(r, u, phase, jb, dccum, mem);
        }
        rs_wave_sync();                                                   // (the planes are complete)

        // ---- pixels: lane = four pixels, four rows a step
        RS_GLOBAL uint8_t* dst = reinterpret_cast<RS_GLOBAL uint8_t*>(r.ptr);
        for (uint32_t ly0 = 0; ly0 < r.V * r.m; ly0 += 4u) {
            uint32_t x, y, v[4];
            const uint32_t n = js_rs_pixels(r, u, lane, ly0, a.bgr, mem, &x, &y, v);
            if (n) rs_store<LAYOUT, DTYPE>(dst + (size_t)y * r.row_pitch, r.plane_pitch, x, n, v, a);
        }
        rs_wave_sync();                                                   // (the next unit's plane writes must not pass these reads)
    }
}

// Grid: six workgroups per compute unit of the CURRENT device (25.5 KiB of LDS each), never more workgroups than there are steps of four units.
// 0, -1 on a launch error or an unknown layout / dtype.
int js_launch_render_ijg_scaled(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsRsRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                                int layout, int dtype, const JsPackArgs& a)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 6u, ((uint64_t)total_units + RS_WAVES - 1u) / RS_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_render_ijg_scaled<JSNOOP_PACK_HWC, JSNOOP_PACK_U8>), dim3(grid), dim3(RS_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_render_ijg_scaled<JSNOOP_PACK_CHW, JSNOOP_PACK_U8>), dim3(grid), dim3(RS_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_render_ijg_scaled<JSNOOP_PACK_HWC, JSNOOP_PACK_F32>), dim3(grid), dim3(RS_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_render_ijg_scaled<JSNOOP_PACK_CHW, JSNOOP_PACK_F32>), dim3(grid), dim3(RS_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, total_units, units_per_wg, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

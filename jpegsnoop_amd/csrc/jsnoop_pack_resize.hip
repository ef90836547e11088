// jsnoop_pack_resize.hip -- k_pack_resize: a rectangle of every listed DIB, resampled to the size its destination asks for, into caller-owned
// device memory.  The sibling of k_pack_rgb (jsnoop_pack.hip): same DIB addressing, same deal of work, same store shapes.
//
// What a pixel is (include/jsnoop_gpu.h): q = (float)((double)S / (double)D) with exact integers S and D that depend on the filter; uint8 output is q
// rounded to nearest even, float output is q * scale[c] + bias[c] as one rounded multiply and one rounded add.  S is summed in integers (32-bit
// horizontally, 64-bit once a vertical weight comes in), so no order of summation can change a bit; the one fp64 division per channel is the last step.
//
// Work: ONE launch for the whole list.  A unit is a segment of JS_RESIZE_SEG pixels of one OUTPUT row, done by one wave, four consecutive pixels per
// lane -- what the stores of the plain pack take.  Units are numbered through a prefix table over the destinations and dealt like k_pack_rgb's: a
// workgroup takes a contiguous share, its four waves interleaved, and everything that depends on the unit only (the destination's record, the output
// row, its vertical footprint and weights) is wave-uniform.
//
// Reads: the ROI's pixel (x, y) is the dword at dib_off + ((img_y - 1 - roi_y - y) * img_x + roi_x + x) * 4; every address below is formed from
// 0 <= x < roi_w, 0 <= y < roi_h, so nothing outside the rectangle is touched -- not the rest of the picture, not the MCU padding.
//   NEAREST, BILINEAR: a lane gathers the one / four dwords of each of its pixels.  Neighbouring lanes read neighbouring or the same dwords when
//     enlarging; when reducing, these two filters skip most of the source by definition.
//   AREA: every source pixel of the footprint counts, so the wave walks the source rows of its output row's vertical footprint and reads the part
//     of each row under its segment coalesced: 16 bytes per lane, 1 KiB per instruction, JS_RESIZE_CHUNK pixels at a time into a 4 KiB stage of
//     LDS that belongs to the wave alone.  The first and last group of a row, where the ROI's edge cuts a 16-byte group, are read dword by dword.
//     Every lane then sums the columns of its four footprints out of LDS with integer weights (the horizontal partial sums stay in the lane's
//     registers: with a wave-private stage no workgroup barrier is needed, only the wave's own), multiplies by the row's weight and adds into
//     64-bit accumulators.  Rows shared by the footprints of two output rows are read twice, the second time out of the caches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"

#define RS_THREADS 256
#define RS_WAVES   (RS_THREADS / 64)

typedef uint32_t rs_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rs_u32x3 __attribute__((ext_vector_type(3)));
typedef float    rs_f32x4 __attribute__((ext_vector_type(4)));
#define RS_GLOBAL __attribute__((address_space(1)))
typedef rs_u32x3 rs_u32x3_a1 __attribute__((aligned(1)));
typedef uint32_t rs_u32_a1   __attribute__((aligned(1)));
typedef rs_f32x4 rs_f32x4_a4 __attribute__((aligned(4)));

// q[j][d]: interpolant of pixel j, DIB channel d (B, G, R).  The stores are pk_store's: 12 contiguous bytes (HWC uint8), one dword per plane (CHW uint8),
// 16-byte vectors (float forms) for four pixels; a tail of n < 4 pixels goes out element by element.  Nothing but addressed elements is written.
template <int LAYOUT, int DTYPE>
__device__ __forceinline__ void rs_store(RS_GLOBAL uint8_t* row /* ptr + oy * row_pitch */, uint64_t plane_pitch, uint32_t x, uint32_t n,
                                         const float (&q)[4][3], const JsPackArgs& a)
{
    if (n == 0u) return;
    if (DTYPE == JSNOOP_PACK_U8) {
        // byte c of v[j] = output channel c of pixel j; rintf is round-to-nearest-even, 0 <= q <= 255
        uint32_t v[4];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t b = (uint32_t)rintf(q[j][0]), g = (uint32_t)rintf(q[j][1]), r = (uint32_t)rintf(q[j][2]);
            v[j] = a.bgr ? (b | (g << 8) | (r << 16)) : (r | (g << 8) | (b << 16));
        }
        if (LAYOUT == JSNOOP_PACK_HWC) {
            RS_GLOBAL uint8_t* o = row + (size_t)x * 3;
            if (n == 4u) {
                rs_u32x3 w;
                w.x = v[0] | (v[1] << 24);
                w.y = (v[1] >> 8) | (v[2] << 16);
                w.z = (v[2] >> 16) | (v[3] << 8);
                *reinterpret_cast<RS_GLOBAL rs_u32x3_a1*>(o) = w;   // (ONE 12-byte store, as in pk_store: the guard bands of the tests catch a widened one)
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
        // out = q * scale[c] + bias[c], c the OUTPUT channel: one rounded multiply, one rounded add, never an FMA
        float f[4][3];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            #pragma unroll
            for (int c = 0; c < 3; c++) f[j][c] = __fadd_rn(__fmul_rn(a.bgr ? q[j][c] : q[j][2 - c], a.scale[c]), a.bias[c]);
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

// the one division of a channel: S < 2^53 and D < 2^53 convert exactly, the quotient is rounded once to double and once to float
__device__ __forceinline__ float rs_quot(uint64_t s, double d) { return (float)((double)s / d); }

// BILINEAR along one axis: P = (2 * o + 1) * r - out; below 0 the first pixel alone, else P div / mod (2 * out); the second pixel is clamped to the edge
__device__ __forceinline__ void rs_lin(uint32_t o, uint32_t r, uint32_t out, uint32_t& i0, uint32_t& i1, uint32_t& frac)
{
    const uint32_t m = (2u * o + 1u) * r;                           // (below 65533 * 65535 < 2^32)
    if (m < out) { i0 = 0u; frac = 0u; }
    else { const uint32_t p = m - out, d = 2u * out; i0 = p / d; frac = p - i0 * d; }
    i1 = min(i0 + 1u, r - 1u);
}

template <int FILTER, int LAYOUT, int DTYPE>
__global__ void __launch_bounds__(RS_THREADS) k_pack_resize(const JsImage* __restrict__ imgs, const uint8_t* __restrict__ dib, const JsResizeRec* __restrict__ recs,
                                                            const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, JsPackArgs a)
{
    __shared__ rs_u32x4 s_stage[FILTER == JSNOOP_RESIZE_AREA ? RS_WAVES * (JS_RESIZE_CHUNK / 4u) : 1u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // this workgroup's share of the units: [u0, u1)
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t u = u0 + wave;
    if (u >= u1) return;
    // the record of the first unit: the last k with unit_base[k] <= u (unit_base[0] = 0, unit_base[nrec] = total_units > u)
    uint32_t k = 0;
    for (uint32_t hi = nrec; hi - k > 1u; ) { const uint32_t mid = (k + hi) >> 1; if (unit_base[mid] <= u) k = mid; else hi = mid; }
    uint32_t kend = 0; bool fresh = true;
    uint32_t kbeg = 0, ow = 1, oh = 1, rw = 1, rh = 1, rx = 0, segs = 1, img_x = 0; uint64_t row_pitch = 0, plane_pitch = 0; RS_GLOBAL uint8_t* dst = nullptr;
    const uint32_t* src0 = nullptr;                                 // the ROI's pixel (0, 0); its row y is src0 - y * img_x
    for (; u < u1; u += RS_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            const JsResizeRec r = recs[k]; const JsImage& im = imgs[r.img];
            ow = r.out_w; oh = r.out_h; rw = r.roi_w; rh = r.roi_h; rx = r.roi_x; img_x = im.img_x; segs = (ow + JS_RESIZE_SEG - 1u) / JS_RESIZE_SEG;
            src0 = reinterpret_cast<const uint32_t*>(dib + im.dib_off) + (size_t)(im.img_y - 1u - r.roi_y) * img_x + rx;
            dst = reinterpret_cast<RS_GLOBAL uint8_t*>(r.ptr); row_pitch = r.row_pitch; plane_pitch = r.plane_pitch;
        }
        const uint32_t lu = u - kbeg, oy = lu / segs, ox0 = (lu - oy * segs) * JS_RESIZE_SEG;
        const uint32_t ox = ox0 + lane * 4u, n = ox < ow ? min(4u, ow - ox) : 0u;
        float q[4][3] = {};
        if (FILTER == JSNOOP_RESIZE_NEAREST) {
            const uint32_t y = ((2u * oy + 1u) * rh) / (2u * oh);
            const uint32_t* src = src0 - (size_t)y * img_x;
            #pragma unroll
            for (int j = 0; j < 4; j++) if ((uint32_t)j < n) {
                const uint32_t p = src[((2u * (ox + j) + 1u) * rw) / (2u * ow)];
                q[j][0] = (float)(p & 0xFFu); q[j][1] = (float)((p >> 8) & 0xFFu); q[j][2] = (float)((p >> 16) & 0xFFu);
            }
        } else if (FILTER == JSNOOP_RESIZE_BILINEAR) {
            uint32_t y0, y1, fy; rs_lin(oy, rh, oh, y0, y1, fy);
            const uint32_t dx = 2u * ow, dy = 2u * oh;
            const uint32_t* s0 = src0 - (size_t)y0 * img_x; const uint32_t* s1 = src0 - (size_t)y1 * img_x;
            const double d = (double)((uint64_t)dx * dy);
            #pragma unroll
            for (int j = 0; j < 4; j++) if ((uint32_t)j < n) {
                uint32_t x0, x1, fx; rs_lin(ox + j, rw, ow, x0, x1, fx);
                const uint32_t p00 = s0[x0], p01 = s0[x1], p10 = s1[x0], p11 = s1[x1];
                #pragma unroll
                for (int c = 0; c < 3; c++) {
                    // a row first: (dx - fx) * a + fx * b <= 65534 * 255 < 2^24; then the two rows with 32 x 32 -> 64-bit products
                    const uint32_t h0 = (dx - fx) * ((p00 >> (8 * c)) & 0xFFu) + fx * ((p01 >> (8 * c)) & 0xFFu);
                    const uint32_t h1 = (dx - fx) * ((p10 >> (8 * c)) & 0xFFu) + fx * ((p11 >> (8 * c)) & 0xFFu);
                    q[j][c] = rs_quot((uint64_t)(dy - fy) * h0 + (uint64_t)fy * h1, d);
                }
            }
        } else {
            // AREA.  In units of 1 / ow source pixel, output column o covers [o * rw, (o + 1) * rw) and source column i covers [i * ow, (i + 1) * ow); rows likewise.
            const uint32_t ylo = oy * rh, yhi = ylo + rh, jy0 = ylo / oh, jy1 = (yhi - 1u) / oh;           // (products below 32767 * 65535 < 2^31)
            uint32_t xlo[4], i0[4], i1[4];
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                xlo[j] = (ox + j) * rw; i0[j] = 1u; i1[j] = 0u;
                if ((uint32_t)j < n) { i0[j] = xlo[j] / ow; i1[j] = (xlo[j] + rw - 1u) / ow; }
            }
            // the source columns under this segment, and where the 16-byte groups of the DIB row fall (DIB rows start 32-byte aligned, img_x is a multiple of 8)
            const uint32_t seg_end = min(ow, ox0 + JS_RESIZE_SEG);
            const uint32_t c_lo = (ox0 * rw) / ow, c_hi = (seg_end * rw - 1u) / ow;
            const int32_t first = (int32_t)((rx + c_lo) & ~3u) - (int32_t)rx;                             // ROI column of the first group's first dword: -3 .. c_lo
            rs_u32x4* stage = s_stage + wave * (JS_RESIZE_CHUNK / 4u);
            const uint32_t* stage32 = reinterpret_cast<const uint32_t*>(stage);
            uint64_t acc[4][3] = {};
            for (uint32_t jy = jy0; jy <= jy1; jy++) {
                const uint32_t wy = min((jy + 1u) * oh, yhi) - max(jy * oh, ylo);
                const uint32_t* src = src0 - (size_t)jy * img_x;
                for (int32_t cs = first; cs <= (int32_t)c_hi; cs += (int32_t)JS_RESIZE_CHUNK) {
                    #pragma unroll
                    for (uint32_t g = 0; g < JS_RESIZE_CHUNK / 256u; g++) {
                        const int32_t col = cs + (int32_t)((g * 64u + lane) * 4u);
                        rs_u32x4 p = { 0u, 0u, 0u, 0u };
                        if (col <= (int32_t)c_hi) {
                            if (col >= 0 && col + 4 <= (int32_t)rw) p = *reinterpret_cast<const rs_u32x4*>(src + col);
                            else {
                                if (col >= 0 && col < (int32_t)rw) p.x = src[col];
                                if (col + 1 >= 0 && col + 1 < (int32_t)rw) p.y = src[col + 1];
                                if (col + 2 >= 0 && col + 2 < (int32_t)rw) p.z = src[col + 2];
                                if (col + 3 >= 0 && col + 3 < (int32_t)rw) p.w = src[col + 3];
                            }
                        }
                        stage[g * 64u + lane] = p;
                    }
                    // the stage is the wave's own: its lanes' writes before its lanes' reads, no other wave involved
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    #pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int32_t a0 = max((int32_t)i0[j], cs), a1 = min((int32_t)i1[j], cs + (int32_t)JS_RESIZE_CHUNK - 1);
                        uint32_t hb = 0, hg = 0, hr = 0;            // each below rw * 255 < 2^24
                        for (int32_t i = a0; i <= a1; i++) {
                            const uint32_t w = min(((uint32_t)i + 1u) * ow, xlo[j] + rw) - max((uint32_t)i * ow, xlo[j]);
                            const uint32_t p = stage32[i - cs];
                            hb += w * (p & 0xFFu); hg += w * ((p >> 8) & 0xFFu); hr += w * ((p >> 16) & 0xFFu);
                        }
                        acc[j][0] += (uint64_t)wy * hb; acc[j][1] += (uint64_t)wy * hg; acc[j][2] += (uint64_t)wy * hr;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
            const double d = (double)((uint64_t)rw * rh);
            #pragma unroll
            for (int j = 0; j < 4; j++) if ((uint32_t)j < n) {
                #pragma unroll
                for (int c = 0; c < 3; c++) q[j][c] = rs_quot(acc[j][c], d);
            }
        }
        rs_store<LAYOUT, DTYPE>(dst + (size_t)oy * row_pitch, plane_pitch, ox, n, q, a);
    }
}

template <int FILTER>
static void rs_launch(hipStream_t st, uint32_t grid, int layout, int dtype, const JsImage* imgs, const uint8_t* dib, const JsResizeRec* recs, const uint32_t* unit_base,
                      uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, const JsPackArgs& a)
{
    if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_pack_resize<FILTER, JSNOOP_PACK_HWC, JSNOOP_PACK_U8>), dim3(grid), dim3(RS_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_pack_resize<FILTER, JSNOOP_PACK_CHW, JSNOOP_PACK_U8>), dim3(grid), dim3(RS_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_HWC) hipLaunchKernelGGL((k_pack_resize<FILTER, JSNOOP_PACK_HWC, JSNOOP_PACK_F32>), dim3(grid), dim3(RS_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else hipLaunchKernelGGL((k_pack_resize<FILTER, JSNOOP_PACK_CHW, JSNOOP_PACK_F32>), dim3(grid), dim3(RS_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
}

// Grid: as js_launch_pack_rgb -- eight workgroups per compute unit of the CURRENT device, never more workgroups than there are steps of four units.
// filter, layout and dtype have been checked by the caller (an unknown one is -1 here all the same).  0, -1 on a launch error.
int js_launch_pack_resize(hipStream_t st, const JsImage* imgs, const uint8_t* dib, const JsResizeRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                          int filter, int layout, int dtype, const JsPackArgs& a)
{
    if (!nrec || !total_units) return 0;
    if ((layout != JSNOOP_PACK_HWC && layout != JSNOOP_PACK_CHW) || (dtype != JSNOOP_PACK_U8 && dtype != JSNOOP_PACK_F32)) return -1;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 8u, ((uint64_t)total_units + RS_WAVES - 1u) / RS_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (filter == JSNOOP_RESIZE_NEAREST) rs_launch<JSNOOP_RESIZE_NEAREST>(st, grid, layout, dtype, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (filter == JSNOOP_RESIZE_BILINEAR) rs_launch<JSNOOP_RESIZE_BILINEAR>(st, grid, layout, dtype, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (filter == JSNOOP_RESIZE_AREA) rs_launch<JSNOOP_RESIZE_AREA>(st, grid, layout, dtype, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

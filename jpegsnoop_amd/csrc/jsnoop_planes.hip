// jsnoop_planes.hip -- k_pack_planes: the retained int16 planes of a decoded batch into caller-owned device memory, one two-dimensional tensor per
// listed (image, component), cropped to the SOF dimensions (FULL) or decimated to the component's own grid (NATIVE), as int16, uint8 or float32.
//
// A plane is the reference's m_pPixValY / Cb / Cr: top-down rows of pw = blk_xmax * 8 int16 samples, blk_ymax * 8 of them, the three planes of an image behind
// each other from plane_off on.  Output element (x, y) of a destination is sample (x * eh, y * ev) of its plane (eh = ev = 1 for FULL); the host resolved
// everything else into the record.  No arithmetic on the samples except the value forms: U8 = min(max((v + 1024) / 8, 0), 255) -- CapYccRange's value; the
// division truncates toward zero, which differs from the arithmetic shift used here only for numerators -7 .. -1, and those clamp to 0 either way --
// and F32 = one multiply and one add, separately rounded, as everywhere in this library.
//
// Work: ONE launch for the whole list, dealt like k_pack_rgb.  A unit is a segment of JS_PLANE_SEG = 512 elements of one OUTPUT row, done by one wave: a lane
// owns eight consecutive elements.  Units are numbered through a prefix table over the records (unit_base, nrec + 1 entries); a workgroup takes a contiguous
// share of the units, its four waves interleaved, finds the record of its first unit by one search of the table and walks on from there: no search and no
// record load per unit.  What depends on the unit alone is wave-uniform and lives in scalar registers.
//
// Loads: rows, plane offsets and plane sizes are multiples of eight samples, and a lane's first source column is a multiple of 8 * eh, so eh = 1 takes ONE
// aligned 16-byte load per lane (a wave-load covers 1 KiB of a plane row) and eh = 2 takes TWO, of which v_perm keeps the even samples; other factors (4:1:1's
// eh = 4, eh = 3) take eight 2-byte loads.  Only rows y * ev are read.  The lanes at the end of a row -- fewer than eight elements left, or a vector that would
// reach past dim_x into the MCU padding -- take the narrow path: one 2-byte load per element, nothing at or past dim_x.
//
// Stores: a lane's eight elements are 8 (U8), 16 (I16) or 2 x 16 (F32) contiguous bytes.  A U8 row may start at any byte and an I16 row at any even one: the
// body relies on the unaligned vector stores global memory takes in the mode the runtime runs gfx9 devices in (k_unaligned_probe; the library refuses to work
// where that does not hold), so there is no head to peel.  The narrow path stores element by element: no byte past the dense row is written, and the bytes
// between the dense row and row_pitch keep their content.  No LDS.  Stores to device memory are vector stores only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"

#define PL_THREADS 256
#define PL_WAVES   (PL_THREADS / 64)

typedef uint32_t pl_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pl_u32x2 __attribute__((ext_vector_type(2)));
typedef float    pl_f32x4 __attribute__((ext_vector_type(4)));
// the same vectors at the alignment the destination guarantees: any byte (U8), an even byte (I16), a dword (F32)
// (destinations are global memory: the address space is spelled out, or a pointer that arrives as a 64-bit number in a record compiles to flat stores)
#define PL_GLOBAL __attribute__((address_space(1)))
typedef pl_u32x2 pl_u32x2_a1 __attribute__((aligned(1)));
typedef pl_u32x4 pl_u32x4_a2 __attribute__((aligned(2)));
typedef pl_f32x4 pl_f32x4_a4 __attribute__((aligned(4)));

// CapYccRange's value of one sample (see the head of the file for the division)
__device__ __forceinline__ uint32_t pl_u8(int v) { return (uint32_t)min(max((v + 1024) >> 3, 0), 255); }

// Output elements x .. x + n - 1 of one row (n <= 8; n < 8 only at the end of a row) as eight int16 in four dwords, element j in half j & 1 of dword j >> 1.
// src: the plane row; element x + j is sample (x + j) * eh; xlim = dim_x.
__device__ __forceinline__ pl_u32x4 pl_load(const int16_t* __restrict__ src, uint32_t x, uint32_t n, uint32_t eh, uint32_t xlim)
{
    pl_u32x4 p = { 0u, 0u, 0u, 0u };
    if (n == 0u) return p;
    const int16_t* s = src + (size_t)x * eh;
    if (n == 8u && (x + 8u) * eh <= xlim && eh <= 2u) {
        if (eh == 1u) p = *reinterpret_cast<const pl_u32x4*>(s);                   // (x is a multiple of 8: aligned)
        else {
            const pl_u32x4 a = reinterpret_cast<const pl_u32x4*>(s)[0], b = reinterpret_cast<const pl_u32x4*>(s)[1];
            // the even samples: the low halves of two neighbouring dwords side by side
            p.x = __builtin_amdgcn_perm(a.y, a.x, 0x05040100u); p.y = __builtin_amdgcn_perm(a.w, a.z, 0x05040100u);
            p.z = __builtin_amdgcn_perm(b.y, b.x, 0x05040100u); p.w = __builtin_amdgcn_perm(b.w, b.z, 0x05040100u);
        }
    } else {
        uint32_t h[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8u; j++) h[j] = j < n ? (uint32_t)(uint16_t)s[(size_t)j * eh] : 0u;
        p.x = h[0] | (h[1] << 16); p.y = h[2] | (h[3] << 16); p.z = h[4] | (h[5] << 16); p.w = h[6] | (h[7] << 16);
    }
    return p;
}

template <int DTYPE>
__device__ __forceinline__ void pl_store(PL_GLOBAL uint8_t* row /* ptr + y * row_pitch */, uint32_t x, uint32_t n, pl_u32x4 p, float scale, float bias)
{
    if (n == 0u) return;
    const uint32_t d[4] = { p.x, p.y, p.z, p.w };
    if (DTYPE == JSNOOP_PLANE_I16) {
        PL_GLOBAL uint8_t* o = row + (size_t)x * 2;
        if (n == 8u) *reinterpret_cast<PL_GLOBAL pl_u32x4_a2*>(o) = p;
        else {
            #pragma unroll
            for (uint32_t j = 0; j < 7u; j++) if (j < n) reinterpret_cast<PL_GLOBAL uint16_t*>(o)[j] = (uint16_t)(d[j >> 1] >> (16u * (j & 1u)));
        }
    } else if (DTYPE == JSNOOP_PLANE_U8) {
        uint32_t b[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8u; j++) b[j] = pl_u8((int)(int16_t)(d[j >> 1] >> (16u * (j & 1u))));
        PL_GLOBAL uint8_t* o = row + x;
        if (n == 8u) {
            pl_u32x2 w;
            w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            *reinterpret_cast<PL_GLOBAL pl_u32x2_a1*>(o) = w;
        } else {
            #pragma unroll
            for (uint32_t j = 0; j < 7u; j++) if (j < n) o[j] = (uint8_t)b[j];
        }
    } else {
        // out = (float)v * scale + bias: one rounded multiply, one rounded add, never an FMA
        float f[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8u; j++) f[j] = __fadd_rn(__fmul_rn((float)(int)(int16_t)(d[j >> 1] >> (16u * (j & 1u))), scale), bias);
        PL_GLOBAL float* o = reinterpret_cast<PL_GLOBAL float*>(row + (size_t)x * 4);
        if (n == 8u) {
            const pl_f32x4 w0 = { f[0], f[1], f[2], f[3] }, w1 = { f[4], f[5], f[6], f[7] };
            PL_GLOBAL pl_f32x4_a4* o4 = reinterpret_cast<PL_GLOBAL pl_f32x4_a4*>(o); o4[0] = w0; o4[1] = w1;
        } else {
            #pragma unroll
            for (uint32_t j = 0; j < 7u; j++) if (j < n) o[j] = f[j];
        }
    }
}

template <int DTYPE>
__global__ void __launch_bounds__(PL_THREADS) k_pack_planes(const int16_t* __restrict__ planes, const JsPlaneRec* __restrict__ recs, const uint32_t* __restrict__ unit_base,
                                                            uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, JsPlaneArgs a)
{
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
    uint32_t kbeg = 0, pw = 0, w = 0, eh = 1, ev = 1, xlim = 0, segs = 1; uint64_t row_pitch = 0; float scale = 1.0f, bias = 0.0f;
    PL_GLOBAL uint8_t* dst = nullptr; const int16_t* src0 = planes;
    for (; u < u1; u += PL_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            const JsPlaneRec r = recs[k];
            pw = r.pw; w = r.w; eh = r.eh; ev = r.ev; xlim = r.xlim; segs = r.segs; row_pitch = r.row_pitch;
            src0 = planes + r.src_off; dst = reinterpret_cast<PL_GLOBAL uint8_t*>(r.ptr);
            scale = r.comp == 0u ? a.scale[0] : r.comp == 1u ? a.scale[1] : a.scale[2];
            bias  = r.comp == 0u ? a.bias[0]  : r.comp == 1u ? a.bias[1]  : a.bias[2];
        }
        const uint32_t lu = u - kbeg, y = lu / segs, x = (lu - y * segs) * JS_PLANE_SEG + lane * 8u;
        const uint32_t n = x < w ? min(8u, w - x) : 0u;
        const pl_u32x4 p = pl_load(src0 + (size_t)y * ev * pw, x, n, eh, xlim);
        pl_store<DTYPE>(dst + (size_t)y * row_pitch, x, n, p, scale, bias);
    }
}

// Grid: eight workgroups per compute unit of the CURRENT device (32 waves per CU: what hides the latency of a kernel with a few dozen registers), never
// more workgroups than there are steps of four units.  0, -1 on a launch error or an unknown dtype.
int js_launch_pack_planes(hipStream_t st, const int16_t* planes, const JsPlaneRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                          int dtype, const JsPlaneArgs& a)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 8u, ((uint64_t)total_units + PL_WAVES - 1u) / PL_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (dtype == JSNOOP_PLANE_I16) hipLaunchKernelGGL((k_pack_planes<JSNOOP_PLANE_I16>), dim3(grid), dim3(PL_THREADS), 0, st, planes, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (dtype == JSNOOP_PLANE_U8) hipLaunchKernelGGL((k_pack_planes<JSNOOP_PLANE_U8>), dim3(grid), dim3(PL_THREADS), 0, st, planes, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (dtype == JSNOOP_PLANE_F32) hipLaunchKernelGGL((k_pack_planes<JSNOOP_PLANE_F32>), dim3(grid), dim3(PL_THREADS), 0, st, planes, recs, unit_base, nrec, total_units, units_per_wg, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

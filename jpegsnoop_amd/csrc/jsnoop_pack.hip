// jsnoop_pack.hip -- k_pack_rgb: the DIBs of a decoded batch into caller-owned device memory, cropped, top-down, three channels.
//
// The DIB is the reference's CDIB: bottom-up rows of img_x BGRA dwords (A = 0), img_x x img_y rounded up to whole MCUs.  Output pixel
// (x, y) of an image, 0 <= x < dim_x, 0 <= y < dim_y, is the dword at dib_off + ((img_y - 1 - y) * img_x + x) * 4.  No arithmetic on the
// colour values except the float form's one multiply and one add (separately rounded, as everywhere in this library).
//
// Work: ONE launch for the whole list.  A unit is a segment of JS_PACK_SEG pixels of one output row, done by one wave: every lane reads two
// 16-byte groups of four pixels, 1 KiB apart, so that a wave's two loads are each 1 KiB of one DIB row, and both are in flight before
// the first store.  Units are numbered through a prefix table over the listed images (unit_base, nrec + 1 entries).  A workgroup takes a
// contiguous share of the units -- its four waves interleaved, 8 KiB of DIB per step -- finds the image of its first unit by a search of
// the prefix table and walks on from there: no search and no descriptor load per unit.  Everything that depends on the unit only is
// wave-uniform and lives in scalar registers.
//
// Stores: four pixels of a lane are 12 contiguous bytes (HWC uint8), one dword per plane (CHW uint8), three or one 16-byte vectors (the
// float forms).  A uint8 destination row may start at any byte: the body then relies on the unaligned vector stores global memory takes in
// the mode the runtime runs gfx9 devices in -- the library refuses to work on a device where k_unaligned_probe shows otherwise -- so there is
// no head to peel.  The tail of a row (dim_x not a multiple of four) is the narrow path: single dword loads, which never touch the MCU
// padding, and single byte / float stores.  Pad bytes between the dense row and row_pitch are never written.  No LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"

#define PK_THREADS 256
#define PK_WAVES   (PK_THREADS / 64)

typedef uint32_t pk_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pk_u32x3 __attribute__((ext_vector_type(3)));
typedef float    pk_f32x4 __attribute__((ext_vector_type(4)));
// the same vectors at the alignment the destination guarantees: any byte (uint8 forms), a dword (float forms)
// (destinations are global memory: the address space is spelled out, or a pointer that arrives as a 64-bit number in a record compiles to flat stores)
#define PK_GLOBAL __attribute__((address_space(1)))
typedef pk_u32x3 pk_u32x3_a1 __attribute__((aligned(1)));
typedef uint32_t pk_u32_a1   __attribute__((aligned(1)));
typedef pk_f32x4 pk_f32x4_a4 __attribute__((aligned(4)));

// up to four pixels from x on; n < 4 only at the end of a row: those lanes read pixel by pixel, nothing past dim_x
__device__ __forceinline__ pk_u32x4 pk_load(const uint32_t* __restrict__ src, uint32_t x, uint32_t n)
{
    pk_u32x4 p = { 0u, 0u, 0u, 0u };
    if (n == 4u) p = *reinterpret_cast<const pk_u32x4*>(src + x);           // (DIB rows start 32-byte aligned, x is a multiple of four)
    else { if (n > 0u) p.x = src[x]; if (n > 1u) p.y = src[x + 1]; if (n > 2u) p.z = src[x + 2]; }
    return p;
}

template <int LAYOUT, int DTYPE>
__device__ __forceinline__ void pk_store(PK_GLOBAL uint8_t* row /* ptr + y * row_pitch */, uint64_t plane_pitch, uint32_t x, uint32_t n,
                                         pk_u32x4 p, const JsPackArgs& a)
{
    if (n == 0u) return;
    // byte c of v[j] = output channel c of pixel j (the DIB's order is B, G, R)
    uint32_t v[4] = { p.x, p.y, p.z, p.w };
    if (!a.bgr) {
        #pragma unroll
        for (int j = 0; j < 4; j++) v[j] = ((v[j] >> 16) & 0xFFu) | (v[j] & 0xFF00u) | ((v[j] & 0xFFu) << 16);
    }
    if (DTYPE == JSNOOP_PACK_U8) {
        if (LAYOUT == JSNOOP_PACK_HWC) {
            PK_GLOBAL uint8_t* o = row + (size_t)x * 3;
            if (n == 4u) {
                pk_u32x3 w;
                w.x = (v[0] & 0xFFFFFFu) | (v[1] << 24);
                w.y = ((v[1] >> 8) & 0xFFFFu) | (v[2] << 16);
                w.z = ((v[2] >> 16) & 0xFFu) | (v[3] << 8);
                // (must stay ONE 12-byte store, global_store_dwordx3: a compiler that widened the three-element vector to four would write a stray dword --
                //  check the assembly after a toolchain change; the guard bands of tests/test_gpu_pack.py catch it)
                *reinterpret_cast<PK_GLOBAL pk_u32x3_a1*>(o) = w;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = (uint8_t)v[j]; o[3 * j + 1] = (uint8_t)(v[j] >> 8); o[3 * j + 2] = (uint8_t)(v[j] >> 16); }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                PK_GLOBAL uint8_t* o = row + (size_t)c * plane_pitch + x;
                if (n == 4u) {
                    *reinterpret_cast<PK_GLOBAL pk_u32_a1*>(o) = ((v[0] >> (8 * c)) & 0xFFu) | (((v[1] >> (8 * c)) & 0xFFu) << 8) |
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
            PK_GLOBAL float* o = reinterpret_cast<PK_GLOBAL float*>(row + (size_t)x * 12);
            if (n == 4u) {
                pk_f32x4 w0 = { f[0][0], f[0][1], f[0][2], f[1][0] }, w1 = { f[1][1], f[1][2], f[2][0], f[2][1] }, w2 = { f[2][2], f[3][0], f[3][1], f[3][2] };
                PK_GLOBAL pk_f32x4_a4* o4 = reinterpret_cast<PK_GLOBAL pk_f32x4_a4*>(o); o4[0] = w0; o4[1] = w1; o4[2] = w2;
            } else {
                #pragma unroll
                for (int j = 0; j < 3; j++) if ((uint32_t)j < n) { o[3 * j] = f[j][0]; o[3 * j + 1] = f[j][1]; o[3 * j + 2] = f[j][2]; }
            }
        } else {
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                PK_GLOBAL float* o = reinterpret_cast<PK_GLOBAL float*>(row + (size_t)c * plane_pitch + (size_t)x * 4);
                if (n == 4u) { pk_f32x4 w = { f[0][c], f[1][c], f[2][c], f[3][c] }; *reinterpret_cast<PK_GLOBAL pk_f32x4_a4*>(o) = w; }
                else {
                    #pragma unroll
                    for (int j = 0; j < 3; j++) if ((uint32_t)j < n) o[j] = f[j][c];
                }
            }
        }
    }
}

template <int LAYOUT, int DTYPE>
__global__ void __launch_bounds__(PK_THREADS) k_pack_rgb(const JsImage* __restrict__ imgs, const uint8_t* __restrict__ dib, const JsPackRec* __restrict__ recs,
                                                         const uint32_t* __restrict__ unit_base, uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, JsPackArgs a)
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
    uint32_t kbeg = 0, dim_x = 0, segs = 1, img_x = 0, last_row = 0; uint64_t row_pitch = 0, plane_pitch = 0; PK_GLOBAL uint8_t* dst = nullptr; const uint32_t* src0 = nullptr;
    for (; u < u1; u += PK_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            const JsPackRec r = recs[k]; const JsImage& im = imgs[r.img];
            dim_x = im.dim_x; img_x = im.img_x; last_row = im.img_y - 1u; segs = (dim_x + JS_PACK_SEG - 1u) / JS_PACK_SEG;
            src0 = reinterpret_cast<const uint32_t*>(dib + im.dib_off);
            dst = reinterpret_cast<PK_GLOBAL uint8_t*>(r.ptr); row_pitch = r.row_pitch; plane_pitch = r.plane_pitch;
        }
        const uint32_t lu = u - kbeg, y = lu / segs, x0 = (lu - y * segs) * JS_PACK_SEG;
        const uint32_t* src = src0 + (size_t)(last_row - y) * img_x;
        PK_GLOBAL uint8_t* row = dst + (size_t)y * row_pitch;
        const uint32_t xa = x0 + lane * 4u, xb = xa + JS_PACK_SEG / 2u;
        const uint32_t na = xa < dim_x ? min(4u, dim_x - xa) : 0u, nb = xb < dim_x ? min(4u, dim_x - xb) : 0u;
        const pk_u32x4 pa = pk_load(src, xa, na), pb = pk_load(src, xb, nb);
        pk_store<LAYOUT, DTYPE>(row, plane_pitch, xa, na, pa, a);
        pk_store<LAYOUT, DTYPE>(row, plane_pitch, xb, nb, pb, a);
    }
}

// Grid: eight workgroups per compute unit of the CURRENT device (32 waves per CU: what hides the latency of a kernel with a few dozen registers), never
// more workgroups than there are steps of four units.  0, -1 on a launch error.
int js_launch_pack_rgb(hipStream_t st, const JsImage* imgs, const uint8_t* dib, const JsPackRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                       int layout, int dtype, const JsPackArgs& a)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 8u, ((uint64_t)total_units + PK_WAVES - 1u) / PK_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_pack_rgb<JSNOOP_PACK_HWC, JSNOOP_PACK_U8>), dim3(grid), dim3(PK_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_U8) hipLaunchKernelGGL((k_pack_rgb<JSNOOP_PACK_CHW, JSNOOP_PACK_U8>), dim3(grid), dim3(PK_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_HWC && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_pack_rgb<JSNOOP_PACK_HWC, JSNOOP_PACK_F32>), dim3(grid), dim3(PK_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else if (layout == JSNOOP_PACK_CHW && dtype == JSNOOP_PACK_F32) hipLaunchKernelGGL((k_pack_rgb<JSNOOP_PACK_CHW, JSNOOP_PACK_F32>), dim3(grid), dim3(PK_THREADS), 0, st, imgs, dib, recs, unit_base, nrec, total_units, units_per_wg, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// jsnoop_encode.hip -- k_encode: 8-bit pictures in device memory to the coefficient arena and the cumulative DC the export reads (the
// arithmetic is libjpeg's integer path and lives in jsnoop_encode_check.h, compiled for host and device; tests/encode_model.py is the definition).
//
// Work: ONE launch for the whole call.  A unit is a run of up to JS_ENC_RUN = 8 consecutive MCUs of one MCU row of one picture, done by one wave; units are
// numbered through a prefix table over the records (unit_base, nrec + 1 entries) and dealt like k_pack_coefs': a workgroup takes a contiguous share, its four
// waves interleaved, finds the record of its first unit by one search and walks on from there.  What depends on the unit only is wave-uniform.  An MCU
// never spans units, so everything below -- the dummy blocks included -- is resolved inside the wave; waves share nothing but the call's tables.
//
// A unit, in four steps, every one through the wave's own LDS (EN_WAVE_BYTES):
//   1. read + colour.  Row by row of the unit's pixel rectangle (up to 128 x 16), lane = pixel: consecutive lanes read consecutive pixels of one source row
//      (one byte load per channel: a wave-load covers one contiguous span of the row at any alignment, pixel stride and pitch), convert with js_enc_ycc and
//      write one byte per component plane.  A pixel right of the picture reads column width - 1, a row below it row height - 1: the replication of the
//      contract, and nothing outside the picture is addressed.
//   2. downsampling (4:2:2, 4:2:0), lane = output column, eight output rows: 2 x 1 with bias (0, 1, ..) or 2 x 2 with bias (1, 2, ..) by output column (a
//      unit starts on an even chroma column: local parity is the picture's).  4:2:0 takes its two source rows from min(cy, ceil(height / 2) - 1): source
//      rows are replicated to an even count only, beyond that the DOWNSAMPLED row repeats.
//   3. forward DCT and quantiser, eight blocks a pass in arena order, eight lanes a block.  Lane (b, r) reads row r of block b (eight bytes), level-shifts,
//      runs the row pass on eight values in registers and writes them as int16 (|v| <= 5793), 16 bytes, into the transpose tile; lane (b, c) reads column c
//      (eight 2-byte reads), runs the column pass in registers, quantises (multiply-high by the entry's reciprocal: exact, jsnoop_encode_check.h) and writes
//      level * q back over the cells it read; lane (b, r) reads row r of the result (16 bytes) and stores it.  A block's tile is 128 bytes at a pitch of
//      EN_BLK_PITCH = 144: the eight blocks of a pass start 36 dwords apart.  A 2-byte access is banked by dword % 32 inside a half of 32 lanes (four blocks):
//      at one row v the four blocks start at banks 0, 4, 8, 12 (the other half: 16, 20, 24, 28) and take four banks each, two lanes a dword -- the column reads
//      and the cell writes of a pass conflict nowhere; at the 128-byte pitch of a dense tile all four blocks of a half would meet on the same four banks.
//      A wave-store writes eight whole arena rows, 1 KiB contiguous, 16 bytes a lane.  Slot 0 is stored as 0; the DC product goes to the wave's DC list.
//   4. cumulative DC.  Lane j owns block j of the unit: a dummy block (a luma block at or beyond the coded part) takes the DC of the nearest block before
//      it in its MCU that is none -- block 0 of an MCU never is one -- and its AC slots were stored as zeros in step 3.  One 2-byte store a lane.
// Integer arithmetic only; no atomics, no scratch; every global store is a vector store.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_encode_check.h"

#define EN_THREADS 256
#define EN_WAVES   (EN_THREADS / 64)
#define EN_PW      128u                      /* pitch of a full-resolution plane: JS_ENC_RUN MCUs of 16 pixels */
#define EN_PLANE   (16u * EN_PW)
#define EN_DW      64u                       /* pitch of a downsampled chroma plane */
#define EN_DOWN    (8u * EN_DW)
#define EN_BLK_PITCH 144u
#define EN_MAX_BLK (JS_ENC_RUN * 6u)
#define EN_OFF_DOWN (3u * EN_PLANE)
#define EN_OFF_TILE (EN_OFF_DOWN + 2u * EN_DOWN)
#define EN_OFF_DC   (EN_OFF_TILE + 8u * EN_BLK_PITCH)
#define EN_WAVE_BYTES (EN_OFF_DC + 128u)     /* 3 planes 6144, 2 downsampled planes 1024, tile 1152, DC list 96 (+ 32): 8448 */

typedef uint32_t en_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t en_u32x2 __attribute__((ext_vector_type(2)));
#define EN_GLOBAL __attribute__((address_space(1)))

static_assert(EN_MAX_BLK <= 64u, "a lane per block of the unit");
static_assert(EN_WAVE_BYTES % 16u == 0 && EN_OFF_TILE % 16u == 0, "16-byte LDS accesses");

__device__ __forceinline__ void en_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(EN_THREADS) k_encode(const JsEncRec* __restrict__ recs, const uint32_t* __restrict__ unit_base, const JsEncTabs* __restrict__ tabs,
                                                       uint32_t nrec, uint32_t total_units, uint32_t units_per_wg, int16_t* __restrict__ coef, int16_t* __restrict__ dccum)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_mem[EN_WAVES * EN_WAVE_BYTES];
    __shared__ JsEncTabs s_tabs;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs); uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tabs);
        for (uint32_t i = threadIdx.x; i < sizeof(JsEncTabs) / 4u; i += EN_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, bl = lane >> 3, r8 = lane & 7u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* mem = s_mem + wave * EN_WAVE_BYTES;
    uint8_t* tile = mem + EN_OFF_TILE;
    int16_t* dc = reinterpret_cast<int16_t*>(mem + EN_OFF_DC);
    const uint32_t u0 = blockIdx.x * units_per_wg, u1 = min(total_units, u0 + units_per_wg);       // (the host sized the grid: no product here passes total_units + units_per_wg)
    uint32_t u = u0 + wave;
    if (u >= u1) return;
    uint32_t k = 0;
    for (uint32_t top = nrec; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (unit_base[mid] <= u) k = mid; else top = mid; }
    uint32_t kbeg = 0, kend = 0; bool fresh = true;
    JsEncRec r;
    for (; u < u1; u += EN_WAVES) {
        if (fresh || u >= kend) {
            while (u >= unit_base[k + 1]) k++;
            fresh = false; kbeg = unit_base[k]; kend = unit_base[k + 1];
            r = recs[k];
        }
        const uint32_t lu = u - kbeg, my = lu / r.runs, m0 = (lu - my * r.runs) * JS_ENC_RUN, nm = min(JS_ENC_RUN, r.mcu_xmax - m0);
        const uint32_t H = r.sub ? 2u : 1u, V = r.sub == 2u ? 2u : 1u, mcu_w = 8u * H, mcu_h = 8u * V;
        const uint32_t x0 = m0 * mcu_w, y0 = my * mcu_h, wpix = nm * mcu_w, nblk = nm * r.bpm;
        const uint64_t blk0 = r.coef_off + ((uint64_t)my * r.mcu_xmax + m0) * r.bpm;

        // ---- 1. read + colour
        for (uint32_t px = lane; px < wpix; px += 64u) {
            const uint64_t xo = (uint64_t)min(x0 + px, r.width - 1u) * r.px_step;
            for (uint32_t row = 0; row < mcu_h; row++) {
                const int64_t yo = (int64_t)min(y0 + row, r.height - 1u) * r.row_step;
                const int c0 = *(const EN_GLOBAL uint8_t*)(r.base[0] + xo + yo);
                if (r.ncomp == 1u) { mem[row * EN_PW + px] = (uint8_t)c0; continue; }
                const int c1 = *(const EN_GLOBAL uint8_t*)(r.base[1] + xo + yo), c2 = *(const EN_GLOBAL uint8_t*)(r.base[2] + xo + yo);
                int y, cb, cr; js_enc_ycc(c0, c1, c2, &y, &cb, &cr);
                mem[row * EN_PW + px] = (uint8_t)y; mem[EN_PLANE + row * EN_PW + px] = (uint8_t)cb; mem[2u * EN_PLANE + row * EN_PW + px] = (uint8_t)cr;
            }
        }
        en_wave_sync();
        // ---- 2. downsampling: lane = output column
        if (r.sub && lane < nm * 8u) {
            const uint32_t bias = lane & 1u, last = (r.height + 1u) / 2u - 1u;
            for (uint32_t c = 0; c < 2u; c++) {
                const uint8_t* p = mem + (c + 1u) * EN_PLANE + 2u * lane; uint8_t* o = mem + EN_OFF_DOWN + c * EN_DOWN + lane;
                for (uint32_t cy = 0; cy < 8u; cy++) {
                    if (r.sub == 1u) o[cy * EN_DW] = (uint8_t)(((uint32_t)p[cy * EN_PW] + p[cy * EN_PW + 1u] + bias) >> 1);
                    else {
                        const uint32_t lr = 2u * min(my * 8u + cy, last) - my * 16u;            // (0 .. 14: the clamp never goes above the unit's first row pair)
                        o[cy * EN_DW] = (uint8_t)(((uint32_t)p[lr * EN_PW] + p[lr * EN_PW + 1u] + p[(lr + 1u) * EN_PW] + p[(lr + 1u) * EN_PW + 1u] + 1u + bias) >> 2);
                    }
                }
            }
        }
        en_wave_sync();
        // ---- 3. forward DCT + quantiser, eight blocks a pass
        const uint32_t ncx = js_enc_coded(r.width, H, H), ncy = js_enc_coded(r.height, V, V);      // luma's coded part, in blocks
        for (uint32_t j0 = 0; j0 < nblk; j0 += 8u) {
            const uint32_t j = j0 + bl; const bool live = j < nblk;
            const uint32_t m = live ? j / r.bpm : 0u, kb = live ? j - m * r.bpm : 0u, nluma = H * V;
            const uint32_t comp = r.ncomp == 1u ? 0u : (kb < nluma ? 0u : kb - nluma + 1u);
            const uint32_t hx = comp ? 0u : kb & (H - 1u), vy = comp ? 0u : kb / H;
            const bool dummy = comp == 0u && ((m0 + m) * H + hx >= ncx || my * V + vy >= ncy);
            const uint8_t* src; uint32_t pitch;
            if (comp == 0u) { src = mem + vy * 8u * EN_PW + (m * H + hx) * 8u; pitch = EN_PW; }
            else if (r.sub == 0u) { src = mem + comp * EN_PLANE + m * 8u; pitch = EN_PW; }
            else { src = mem + EN_OFF_DOWN + (comp - 1u) * EN_DOWN + m * 8u; pitch = EN_DW; }
            const en_u32x2 raw = *reinterpret_cast<const en_u32x2*>(src + r8 * pitch);
            int d[8];
            #pragma unroll
            for (int i = 0; i < 4; i++) { d[i] = (int)((raw.x >> (8 * i)) & 255u) - 128; d[4 + i] = (int)((raw.y >> (8 * i)) & 255u) - 128; }
            js_enc_fdct_pass<true>(d);
            uint8_t* tb = tile + bl * EN_BLK_PITCH;
            #define EN_PK(a, b) (((uint32_t)(a) & 0xFFFFu) | ((uint32_t)(b) << 16))
            *reinterpret_cast<en_u32x4*>(tb + r8 * 16u) = en_u32x4{ EN_PK(d[0], d[1]), EN_PK(d[2], d[3]), EN_PK(d[4], d[5]), EN_PK(d[6], d[7]) };
            #undef EN_PK
            en_wave_sync();
            #pragma unroll
            for (int v = 0; v < 8; v++) d[v] = *reinterpret_cast<const int16_t*>(tb + v * 16 + r8 * 2u);
            js_enc_fdct_pass<false>(d);
            const uint32_t t = comp ? 1u : 0u;
            #pragma unroll
            for (int v = 0; v < 8; v++) {
                const uint32_t n = (uint32_t)v * 8u + r8;
                int p = js_enc_quant(d[v], s_tabs.q[t][n], s_tabs.recip[t][n]);
                if (n == 0u) { if (live) dc[j] = (int16_t)p; p = 0; }
                *reinterpret_cast<int16_t*>(tb + v * 16 + r8 * 2u) = (int16_t)(dummy ? 0 : p);
            }
            en_wave_sync();
            const en_u32x4 out = *reinterpret_cast<const en_u32x4*>(tb + r8 * 16u);
            if (live) *(EN_GLOBAL en_u32x4*)(coef + (blk0 + j) * 64u + r8 * 8u) = out;
            en_wave_sync();                                               // (the next pass's tile writes must not pass these reads)
        }
        // ---- 4. cumulative DC: lane = block of the unit
        if (lane < nblk) {
            const uint32_t m = lane / r.bpm, kb = lane - m * r.bpm;
            uint32_t from = lane;
            if (r.sub && kb < H * V) {
                uint32_t q = kb;
                while (q && ((m0 + m) * H + (q & (H - 1u)) >= ncx || my * V + q / H >= ncy)) q--;
                from = lane - (kb - q);
            }
            *(EN_GLOBAL int16_t*)(dccum + blk0 + lane) = dc[from];
        }
        en_wave_sync();                                                   // (the next unit's plane and DC writes must not pass these reads)
    }
}

// Grid: four workgroups per compute unit of the CURRENT device (33 KiB + the tables of LDS each), never more workgroups than there are steps of four units.
// 0, -1 on a launch error.
int js_launch_encode(hipStream_t st, const JsEncRec* recs, const uint32_t* unit_base, const JsEncTabs* tabs, uint32_t nrec, uint32_t total_units, int16_t* coef, int16_t* dccum)
{
    if (!nrec || !total_units) return 0;
    int devi = 0, cus = 0;
    if (hipGetDevice(&devi) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || cus <= 0) return -1;
    const uint64_t want = std::min<uint64_t>((uint64_t)cus * 4u, ((uint64_t)total_units + EN_WAVES - 1u) / EN_WAVES);
    const uint32_t units_per_wg = (uint32_t)(((uint64_t)total_units + want - 1u) / want), grid = (uint32_t)(((uint64_t)total_units + units_per_wg - 1u) / units_per_wg);
    if ((uint64_t)grid * units_per_wg > 0xFFFFFFFFull) return -1;                                   // (u0 of the last workgroup must not wrap)
    hipLaunchKernelGGL(k_encode, dim3(grid), dim3(EN_THREADS), 0, st, recs, unit_base, tabs, nrec, total_units, units_per_wg, coef, dccum);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

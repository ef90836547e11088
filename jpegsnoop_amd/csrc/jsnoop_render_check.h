// jsnoop_render_check.h -- the arithmetic of jsnoop_batch_pack_ijg that is not a device call: which images are renderable, the checks of a destination,
// records and the unit plan -- and the integer kernels of the render itself (one jidctint step, the two upsampling formulas, the colour lines) together
// with the job list of a unit (which arena blocks a wave transforms and where in its LDS the samples go, halo included), compiled for host AND device:
// k_render_ijg (jsnoop_render.hip) calls the very functions tests/cpp/render_check.cpp runs as a plain host program.  Errors go through js_set_error.
// tests/ijg_model.py is the definition.
//
// Bounds (tests/cpp/render_check.cpp walks the ones marked *):
//   every job of every unit names an arena block of its own image *, and its samples land inside the plane they belong to * -- own samples on own cells,
//   halo samples on halo cells, no cell written twice *.
//   a chroma cell the filter reads is either an own cell or a halo cell some job of the unit wrote *: the clamp of the contract is applied to the INDEX
//   (js_ren_clamp_col / _row), so a neighbour outside the picture is never looked up.
//   arithmetic: the transform is written on uint32_t -- sums and products wrap modulo 2^32 as the contract says, and nothing is undefined for any int16 input.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"
#include "jsnoop_pack_check.h"

#if defined(__HIPCC__)
#define JS_REN_HD __host__ __device__ __forceinline__
#else
#define JS_REN_HD inline
#endif

// ---------------------------------------------------------------------------------------------- the transform (host and device)
// One 1-D step of jidctint (CONST_BITS 13, PASS1_BITS 2) over v[0..7], in place, descaled by SHIFT (11: pass 1, the columns; 18: pass 2, the rows).
template <int SHIFT>
JS_REN_HD void js_ren_idct_step(int32_t v[8])
{
    typedef uint32_t U;
    const U v0 = (U)v[0], v1 = (U)v[1], v2 = (U)v[2], v3 = (U)v[3], v4 = (U)v[4], v5 = (U)v[5], v6 = (U)v[6], v7 = (U)v[7];
    U z1 = (v2 + v6) * 4433u;
    const U t2 = z1 - v6 * 15137u, t3 = z1 + v2 * 6270u, t0 = (v0 + v4) << 13, t1 = (v0 - v4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    U a = v7, b = v5, c = v3, d = v1;
    z1 = a + d; U z2 = b + c, z3 = a + c, z4 = b + d; const U z5 = (z3 + z4) * 9633u;
    a *= 2446u; b *= 16819u; c *= 25172u; d *= 12299u;
    z1 *= (U)-7373; z2 *= (U)-20995; z3 = z3 * (U)-16069 + z5; z4 = z4 * (U)-3196 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    const U r = 1u << (SHIFT - 1);
    v[0] = (int32_t)(t10 + d + r) >> SHIFT; v[7] = (int32_t)(t10 - d + r) >> SHIFT;
    v[1] = (int32_t)(t11 + c + r) >> SHIFT; v[6] = (int32_t)(t11 - c + r) >> SHIFT;
    v[2] = (int32_t)(t12 + b + r) >> SHIFT; v[5] = (int32_t)(t12 - b + r) >> SHIFT;
    v[3] = (int32_t)(t13 + a + r) >> SHIFT; v[4] = (int32_t)(t13 - a + r) >> SHIFT;
}
// the sample of a pass-2 result: a true saturation (|result| < 2^14, the sum cannot wrap)
JS_REN_HD uint32_t js_ren_sample(int32_t r) { const int32_t s = r + 128; return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s)); }
// 2 x 1: p = the sample, l / r = its clamped neighbours -> the two output columns
JS_REN_HD void js_ren_h2v1(uint32_t l, uint32_t p, uint32_t r, uint32_t* even, uint32_t* odd) { *even = (3u * p + l + 1u) >> 2; *odd = (3u * p + r + 2u) >> 2; }
// 2 x 2: the column sums s = 3 p[j] + p[j -+ 1] first, then along the row
JS_REN_HD uint32_t js_ren_h2v2_sum(uint32_t near, uint32_t far) { return 3u * near + far; }
JS_REN_HD void js_ren_h2v2(uint32_t l, uint32_t s, uint32_t r, uint32_t* even, uint32_t* odd) { *even = (3u * s + l + 8u) >> 4; *odd = (3u * s + r + 7u) >> 4; }
JS_REN_HD uint32_t js_ren_clamp8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// Y, Cb, Cr 0..255 -> byte 0 = R, 1 = G, 2 = B (libjpeg's ycc_rgb tables, SCALEBITS 16; >> is arithmetic)
JS_REN_HD uint32_t js_ren_rgb(uint32_t y, uint32_t cb_, uint32_t cr_)
{
    const int cb = (int)cb_ - 128, cr = (int)cr_ - 128, yy = (int)y;
    const uint32_t r = js_ren_clamp8(yy + ((91881 * cr + 32768) >> 16));
    const uint32_t g = js_ren_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const uint32_t b = js_ren_clamp8(yy + ((116130 * cb + 32768) >> 16));
    return r | (g << 8) | (b << 16);
}

// ---------------------------------------------------------------------------------------------- a unit's LDS and its job list (host and device)
// A unit is a run of up to JS_REN_RUN MCUs of one MCU row.  Its wave holds, in JS_REN_WAVE_BYTES of LDS:
//   the luma rectangle, 16 rows at a pitch of 128 bytes (sample (x, y) of the unit at y * 128 + x);
//   two chroma planes of 10 rows at a pitch of 80: local row lr = chroma row - (8 my - 1), local column lc = chroma column - (8 m0 - 1), the cell at
//   lr * 80 + 7 + lc.  Own samples are lr 1..8, lc 1..8 nm (a block's row starts on an 8-byte boundary); lr 0 / 9 and lc 0 / 8 nm + 1 are the halo;
//   the transpose tile, eight blocks of 64 dwords at a pitch of 72 dwords.
#define JS_REN_RUN      8u
#define JS_REN_Y_PITCH  128u
#define JS_REN_Y_BYTES  (16u * JS_REN_Y_PITCH)
#define JS_REN_C_PITCH  80u
#define JS_REN_C_BYTES  (10u * JS_REN_C_PITCH)
#define JS_REN_OFF_C    JS_REN_Y_BYTES
#define JS_REN_OFF_TILE (JS_REN_OFF_C + 2u * JS_REN_C_BYTES)
#define JS_REN_BLK_PITCH 72u           /* dwords */
#define JS_REN_WAVE_BYTES (JS_REN_OFF_TILE + 8u * JS_REN_BLK_PITCH * 4u)     /* 2048 + 1600 + 2304 = 5952 */
#define JS_REN_MAX_JOBS (JS_REN_RUN * 6u + 2u * (2u + 2u * (JS_REN_RUN + 2u)))

// jsnoop_batch_pack_ijg (k_render_ijg): one record per listed destination, everything the kernel needs of its image resolved on the host, and a prefix table in
// which destination k owns mcu_ymax * runs units (runs = ceil(mcu_xmax / JS_REN_RUN)).  H x V: luma's sampling (1 x 1, 2 x 1, 2 x 2); bpm = H V + 2, or 1 (grey).
struct JsRenRec { uint64_t ptr, row_pitch, plane_pitch, coef_off; uint32_t dim_x, dim_y, ncomp, H, V, mcu_xmax, mcu_ymax, runs, bpm, reserved; };

JS_REN_HD uint32_t js_ren_c_cell(uint32_t comp /*1, 2*/, uint32_t lr, uint32_t lc) { return JS_REN_OFF_C + (comp - 1u) * JS_REN_C_BYTES + lr * JS_REN_C_PITCH + 7u + lc; }
// jobs of a unit of nm MCUs: its own blocks, then -- where chroma is upsampled -- per chroma component the left and the right neighbour block and, for 2 x 2,
// the nm + 2 blocks above and the nm + 2 below
JS_REN_HD uint32_t js_ren_halo_per_comp(const JsRenRec& r, uint32_t nm) { return r.ncomp == 3u && r.H == 2u ? 2u + (r.V == 2u ? 2u * (nm + 2u) : 0u) : 0u; }
JS_REN_HD uint32_t js_ren_jobs(const JsRenRec& r, uint32_t nm) { return nm * r.bpm + 2u * js_ren_halo_per_comp(r, nm); }
// Job jb of the unit (my, m0, nm), as lane r8 of the eight lanes that share it sees it: exists -- the block is there (its eight rows are loaded and transformed);
// blk -- its arena row, relative to the image's first; mask -- bit i set: sample i of result row r8 is kept, at byte dst0 + i of the wave's LDS.
struct JsRenJob { uint32_t exists, mask, dst0; uint64_t blk; };
JS_REN_HD JsRenJob js_ren_job(const JsRenRec& r, uint32_t my, uint32_t m0, uint32_t nm, uint32_t jb, uint32_t r8)
{
    JsRenJob j; j.exists = 0u; j.mask = 0u; j.dst0 = 0u; j.blk = 0u;
    const uint32_t nown = nm * r.bpm, nluma = r.ncomp == 1u ? 1u : r.H * r.V;
    if (jb < nown) {
        const uint32_t m = jb / r.bpm, kb = jb - m * r.bpm;
        j.exists = 1u; j.mask = 0xFFu; j.blk = ((uint64_t)my * r.mcu_xmax + m0 + m) * r.bpm + kb;
        if (kb < nluma) { const uint32_t hx = kb & (r.H - 1u), vy = kb / r.H; j.dst0 = (vy * 8u + r8) * JS_REN_Y_PITCH + (m * r.H + hx) * 8u; }
        else j.dst0 = js_ren_c_cell(kb - nluma + 1u, 1u + r8, 1u + m * 8u);
        return j;
    }
    const uint32_t per = js_ren_halo_per_comp(r, nm), h = jb - nown;
    if (h >= 2u * per) return j;
    const uint32_t ci = h >= per ? 1u : 0u, s = h - ci * per, comp = ci + 1u;
    uint32_t mx, myy, lr, lc, row = 8u /* which result row is kept; 8: every row, one sample each */, one = 8u /* which sample; 8: all */;
    if (s == 0u) { if (m0 == 0u) return j; mx = m0 - 1u; myy = my; lc = 0u; one = 7u; lr = 1u + r8; }
    else if (s == 1u) { if (m0 + nm >= r.mcu_xmax) return j; mx = m0 + nm; myy = my; lc = nm * 8u + 1u; one = 0u; lr = 1u + r8; }
    else {
        uint32_t t = s - 2u;
        if (t < nm + 2u) { if (my == 0u) return j; myy = my - 1u; row = 7u; lr = 0u; }
        else { t -= nm + 2u; if (my + 1u >= r.mcu_ymax) return j; myy = my + 1u; row = 0u; lr = 9u; }
        if (m0 + t < 1u || m0 + t - 1u >= r.mcu_xmax) return j;
        mx = m0 + t - 1u;
        if (t == 0u) { lc = 0u; one = 7u; } else if (t == nm + 1u) { lc = nm * 8u + 1u; one = 0u; } else lc = 1u + (t - 1u) * 8u;
    }
    j.exists = 1u; j.blk = ((uint64_t)myy * r.mcu_xmax + mx) * r.bpm + nluma + ci;
    if (row == 8u || row == r8) { j.mask = one == 8u ? 0xFFu : 1u << one; j.dst0 = js_ren_c_cell(comp, lr, lc) - (one == 8u ? 0u : one); }
    return j;
}
// the cell of chroma sample (column i, row j of the component's plane, any integers) as the filter reads it: the index clamped to the real extent
// (dw x dh), then made local to the unit
JS_REN_HD uint32_t js_ren_clamp_col(int i, uint32_t dw, uint32_t m0) { const uint32_t g = i < 0 ? 0u : ((uint32_t)i >= dw ? dw - 1u : (uint32_t)i); return g + 1u - m0 * 8u; }
JS_REN_HD uint32_t js_ren_clamp_row(int j, uint32_t dh, uint32_t my) { const uint32_t g = j < 0 ? 0u : ((uint32_t)j >= dh ? dh - 1u : (uint32_t)j); return g + 1u - my * 8u; }

// four upsampled samples of one chroma component for pixels 2 i0 .. 2 i0 + 3 of picture row y (H = 2): p = the component's plane in the wave's LDS (cell (0, 0) at p + 7)
JS_REN_HD void js_ren_chroma4(const uint8_t* p, uint32_t V, uint32_t y, uint32_t i0, uint32_t dw, uint32_t dh, uint32_t my, uint32_t m0, uint32_t out[4])
{
    if (dw <= 2u) {                                                   // libjpeg does not interpolate such a plane: replication
        const uint32_t lr = js_ren_clamp_row((int)(V == 2u ? y >> 1 : y), dh, my);
        const uint32_t a = p[lr * JS_REN_C_PITCH + 7u + js_ren_clamp_col((int)i0, dw, m0)], b = p[lr * JS_REN_C_PITCH + 7u + js_ren_clamp_col((int)i0 + 1, dw, m0)];
        out[0] = a; out[1] = a; out[2] = b; out[3] = b;
        return;
    }
    uint32_t lc[4], s[4];
    for (int k = 0; k < 4; k++) lc[k] = 7u + js_ren_clamp_col((int)i0 - 1 + k, dw, m0);
    if (V == 2u) {
        const int j = (int)(y >> 1);
        const uint32_t near = js_ren_clamp_row(j, dh, my) * JS_REN_C_PITCH, far = js_ren_clamp_row((y & 1u) ? j + 1 : j - 1, dh, my) * JS_REN_C_PITCH;
            for (int k = 0; k < 4; k++) s[k] = js_ren_h2v2_sum(p[near + lc[k]], p[far + lc[k]]);
        uint32_t e, o;
        js_ren_h2v2(s[0], s[1], s[2], &e, &o); out[0] = e; out[1] = o;
        js_ren_h2v2(s[1], s[2], s[3], &e, &o); out[2] = e; out[3] = o;
    } else {
        const uint32_t row = js_ren_clamp_row((int)y, dh, my) * JS_REN_C_PITCH;
            for (int k = 0; k < 4; k++) s[k] = p[row + lc[k]];
        uint32_t e, o;
        js_ren_h2v1(s[0], s[1], s[2], &e, &o); out[0] = e; out[1] = o;
        js_ren_h2v1(s[1], s[2], s[3], &e, &o); out[2] = e; out[3] = o;
    }
}

// ---------------------------------------------------------------------------------------------- renderable, plan (host)
// 0 when image i renders; -1 + the reason.  Host arithmetic on the descriptor alone.
inline int js_ren_renderable(const JsImage& im, int i, uint32_t* H = nullptr, uint32_t* V = nullptr)
{
    if (im.precision != 8u) { js_set_error("pack_ijg: image %d has a sample precision of %u bits, 8 are rendered", i, im.precision); return -1; }
    if (im.ncomp != 1u && im.ncomp != 3u) { js_set_error("pack_ijg: image %d has %u components, 1 or 3 are rendered", i, im.ncomp); return -1; }
    if (!im.dim_x || !im.dim_y || !im.mcu_xmax || !im.mcu_ymax || !im.blk_per_mcu || im.blk_per_mcu > JS_MAX_BLK_PER_MCU) { js_set_error("pack_ijg: image %d has no decoded geometry", i); return -1; }
    uint32_t h = 1, v = 1;
    if (im.ncomp == 1u) {
        if (im.blk_per_mcu != 1u || im.mcu_w != 8u || im.mcu_h != 8u) { js_set_error("pack_ijg: image %d: one component with %u blocks per MCU of %u x %u, one 8 x 8 block is rendered", i, im.blk_per_mcu, im.mcu_w, im.mcu_h); return -1; }
    } else {
        h = im.samp_h[1]; v = im.samp_v[1];
        if (im.samp_h[2] != 1u || im.samp_v[2] != 1u || im.samp_h[3] != 1u || im.samp_v[3] != 1u) {
            js_set_error("pack_ijg: image %d: chroma sampling %u x %u / %u x %u, 1 x 1 is rendered", i, im.samp_h[2], im.samp_v[2], im.samp_h[3], im.samp_v[3]); return -1; }
        if (!((h == 1u && v == 1u) || (h == 2u && v == 1u) || (h == 2u && v == 2u))) { js_set_error("pack_ijg: image %d: luma sampling %u x %u, 1 x 1 (4:4:4), 2 x 1 (4:2:2) and 2 x 2 (4:2:0) are rendered", i, h, v); return -1; }
        if (im.blk_per_mcu != h * v + 2u || im.mcu_w != 8u * h || im.mcu_h != 8u * v) { js_set_error("pack_ijg: image %d: %u blocks per MCU of %u x %u do not belong to sampling %u x %u", i, im.blk_per_mcu, im.mcu_w, im.mcu_h, h, v); return -1; }
        for (uint32_t y = 0; y < v; y++) for (uint32_t x = 0; x < h; x++) {
            const uint32_t j = y * h + x;
            if (im.blk_comp[j] != 1u || im.blk_ch[j] != x || im.blk_cv[j] != y) { js_set_error("pack_ijg: image %d: unexpected block order inside the MCU", i); return -1; }
        }
        if (im.blk_comp[h * v] != 2u || im.blk_comp[h * v + 1u] != 3u) { js_set_error("pack_ijg: image %d: unexpected block order inside the MCU", i); return -1; }
    }
    if (im.mcu_xmax != (im.dim_x + 8u * h - 1u) / (8u * h) || im.mcu_ymax != (im.dim_y + 8u * v - 1u) / (8u * v) || im.dim_x > 65535u || im.dim_y > 65535u ||
        (uint64_t)im.total_blocks != (uint64_t)im.mcu_xmax * im.mcu_ymax * im.blk_per_mcu) { js_set_error("pack_ijg: image %d: the MCU grid does not belong to %u x %u pixels", i, im.dim_x, im.dim_y); return -1; }
    if (H) *H = h;
    if (V) *V = v;
    return 0;
}
inline uint64_t js_ren_units(const JsImage& im) { return (uint64_t)im.mcu_ymax * ((im.mcu_xmax + JS_REN_RUN - 1u) / JS_REN_RUN); }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_pack_import_spec(.., "pack_ijg").  The destination checks are jsnoop_batch_pack's.
inline int js_ren_plan(const JsImage* imgs, size_t nimg, const JsnoopPackSpec& s, const int* images, int n, const JsnoopPackDst* dst, JsRenRec* recs, uint32_t* unit_base)
{
    uint64_t units = 0;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_ijg: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        uint32_t H = 1, V = 1;
        if (js_ren_renderable(im, i, &H, &V)) return -1;
        const JsnoopPackDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack_ijg: destination %d (image %d) is NULL", k, i); return -1; }
        const uint64_t dense_row = js_pack_dense_row(im, s), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack_ijg: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        const uint64_t dense_plane = (uint64_t)im.dim_y * row_pitch;
        uint64_t plane_pitch = dense_plane;
        if (s.layout == JSNOOP_PACK_CHW) {
            if (d.plane_pitch) plane_pitch = d.plane_pitch;
            if (plane_pitch < dense_plane) { js_set_error("pack_ijg: plane_pitch %llu of destination %d (image %d) is below the dense plane of %llu bytes", (unsigned long long)d.plane_pitch, k, i, (unsigned long long)dense_plane); return -1; }
        }
        if (s.dtype == JSNOOP_PACK_F32 && (((uint64_t)(uintptr_t)d.ptr | row_pitch | plane_pitch) & 3u)) {
            js_set_error("pack_ijg: float32 destination %d (image %d): pointer and pitches must be multiples of 4", k, i); return -1; }
        JsRenRec& r = recs[k];
        memset(&r, 0, sizeof r);
        r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch; r.plane_pitch = plane_pitch; r.coef_off = im.coef_off;
        r.dim_x = im.dim_x; r.dim_y = im.dim_y; r.ncomp = im.ncomp; r.H = H; r.V = V; r.mcu_xmax = im.mcu_xmax; r.mcu_ymax = im.mcu_ymax;
        r.runs = (im.mcu_xmax + JS_REN_RUN - 1u) / JS_REN_RUN; r.bpm = im.blk_per_mcu;
        unit_base[k] = (uint32_t)units; units += js_ren_units(im);
        if (units >= 0x7FFFFFFFull) { js_set_error("pack_ijg: more than 2^31 units of work in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}

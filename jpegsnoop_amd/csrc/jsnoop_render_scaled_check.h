// jsnoop_render_scaled_check.h -- the arithmetic of jsnoop_batch_pack_ijg_scaled that is not a device call: the reduced sizes, the transform size of a component,
// the checks of a destination, records and the unit plan -- and the integer kernels of the reduced render (the 4 x 4 and 2 x 2 steps of jidctred, the 1 x 1,
// the 4:2:2 chroma look-up) together with the job list of a unit (which arena blocks a wave transforms at which size and where in its LDS the samples go, halo
// included), compiled for host AND device: k_render_ijg_scaled (jsnoop_render_scaled.hip) calls the very functions tests/cpp/render_scaled_check.cpp runs as
// a plain host program.  The 8 x 8 step, the h2v1 formula, the colour lines and `renderable` are jsnoop_render_check.h's.  tests/ijg_scaled_model.py is the
// definition.
//
// Bounds (tests/cpp/render_scaled_check.cpp walks the ones marked *):
//   every job of every unit names an arena block of its own image *; its samples land inside the plane of its component *, own samples on own cells, halo
//   samples on the two halo columns, no cell written twice *; a component transformed 1 x 1 reads dccum alone *.
//   a cell step 2 reads was written by a job of the unit *: js_rs_chroma4 clamps the chroma INDEX to the component's real width before it makes it local.
//   workspace rows: job jg of a group and its row k sit at row jg * n + k < 64 *.
//   arithmetic: the steps are written on uint32_t -- sums and products wrap modulo 2^32 as the contract says, nothing is undefined for any int16 input.
#pragma once
#include "jsnoop_render_check.h"

// ---------------------------------------------------------------------------------------------- the reduced transforms (host and device)
// One 1-D step of jidctred's 4 x 4 (CONST_BITS 13, PASS1_BITS 2) on v[0..7] -> out[0..3], descaled by SHIFT (12: pass 1, 19: pass 2).  v[4] is not read.
template <int SHIFT>
JS_REN_HD void js_rs_step4(const int32_t v[8], int32_t out[4])
{
    typedef uint32_t U;
    const U v0 = (U)v[0], v1 = (U)v[1], v2 = (U)v[2], v3 = (U)v[3], v5 = (U)v[5], v6 = (U)v[6], v7 = (U)v[7];
    const U t0 = v0 << 14, t2 = v2 * 15137u - v6 * 6270u, t10 = t0 + t2, t12 = t0 - t2;
    const U a = v7 * (U)-1730 + v5 * 11893u + v3 * (U)-17799 + v1 * 8697u;
    const U b = v7 * (U)-4176 + v5 * (U)-4926 + v3 * 7373u + v1 * 20995u;
    const U r = 1u << (SHIFT - 1);
    out[0] = (int32_t)(t10 + b + r) >> SHIFT; out[3] = (int32_t)(t10 - b + r) >> SHIFT;
    out[1] = (int32_t)(t12 + a + r) >> SHIFT; out[2] = (int32_t)(t12 - a + r) >> SHIFT;
}
// ... of the 2 x 2 (13: pass 1, 20: pass 2).  v[2], v[4], v[6] are not read.
template <int SHIFT>
JS_REN_HD void js_rs_step2(const int32_t v[8], int32_t out[2])
{
    typedef uint32_t U;
    const U t10 = (U)v[0] << 15, t0 = (U)v[7] * (U)-5906 + (U)v[5] * 6967u + (U)v[3] * (U)-10426 + (U)v[1] * 29692u, r = 1u << (SHIFT - 1);
    out[0] = (int32_t)(t10 + t0 + r) >> SHIFT; out[1] = (int32_t)(t10 - t0 + r) >> SHIFT;
}
// the 1 x 1: DESCALE(dc, 3) of the block's cumulative DC (an int16: the sum cannot wrap)
JS_REN_HD int32_t js_rs_dc(int32_t dc) { return (dc + 4) >> 3; }
// which rows of a block pass 1 of an n x n transform reads -- the 16-byte arena segments a job fetches -- and which columns it transforms: all eight (8),
// all but 4 (4), {0, 1, 3, 5, 7} (2)
JS_REN_HD bool js_rs_needs(uint32_t n, uint32_t i) { return n == 8u || (n == 4u ? i != 4u : (i == 0u || (i & 1u))); }

// ---------------------------------------------------------------------------------------------- a unit's LDS and its job list (host and device)
// m = 8 / denom.  Component sizes: luma ny = m; chroma nc = m, or 2 m for 4:2:0 (jdmaster's rule, js_rs_size).  An MCU gives H m x V m pixels; a unit is a
// run of up to run = 64 / (H m) MCUs of one MCU row, so 64 pixels wide and V m <= 8 rows high.  Its wave holds, in JS_RS_WAVE_BYTES of LDS:
//   three byte planes (Y, Cb, Cr) of 8 rows at a pitch of 80: sample (x, y) of the component's part of the unit at y * 80 + 8 + x.  Luma, 4:4:4 and 4:2:0
//   chroma fill 64 columns (4:2:0 chroma is transformed at the MCU's output size: nothing is upsampled); 4:2:2 chroma fills 32 and, at denom 2 and 4, the
//   halo columns x = -1 and x = 32 (or nm * nc of a short unit);
//   the load tile: eight blocks of 64 dwords at a pitch of 72 dwords, where pass 1 turns rows into columns;
//   the workspace: 64 rows of 8 dwords -- a group of 64 / n jobs, n rows each -- with 8 dwords of padding behind every 8 rows (row q at dword 8 q + 8 (q >> 3)).
#define JS_RS_PITCH       80u
#define JS_RS_PLANE_BYTES (8u * JS_RS_PITCH)
#define JS_RS_OFF_TILE    (3u * JS_RS_PLANE_BYTES)
#define JS_RS_BLK_PITCH   72u          /* dwords */
#define JS_RS_OFF_WS      (JS_RS_OFF_TILE + 8u * JS_RS_BLK_PITCH * 4u)
#define JS_RS_WS_DWORDS   (64u * 8u + 8u * 8u)
#define JS_RS_WAVE_BYTES  (JS_RS_OFF_WS + JS_RS_WS_DWORDS * 4u)                 /* 1920 + 2304 + 2304 = 6528 */
JS_REN_HD uint32_t js_rs_ws_row(uint32_t q) { return 8u * q + 8u * (q >> 3); }  // dword of workspace row q

// One record per listed destination, everything the kernel needs of its image resolved on the host, and a prefix table in which destination k owns
// mcu_ymax * runs units.  out_x / out_y: the reduced picture; dwc: the real width of a chroma plane in samples (the filter's clamp).
struct JsRsRec { uint64_t ptr, row_pitch, plane_pitch, coef_off; uint32_t out_x, out_y, ncomp, H, V, mcu_xmax, mcu_ymax, runs, bpm, m, ny, nc, run, dwc, reserved[2]; };

// jdmaster's transform size of a component sampled h x v in a frame of hmax x vmax at m = 8 / denom
JS_REN_HD uint32_t js_rs_size(uint32_t m, uint32_t hmax, uint32_t vmax, uint32_t h, uint32_t v)
{
    uint32_t n = m;
    while (n < 8u && (hmax * m) % (h * n * 2u) == 0u && (vmax * m) % (v * n * 2u) == 0u) n *= 2u;
    return n;
}
// 4:2:2 at denom 2 and 4: the one case with a filter, so with a halo
JS_REN_HD bool js_rs_filtered(const JsRsRec& r) { return r.ncomp == 3u && r.H == 2u && r.V == 1u && r.m > 1u; }
// phase 0: the luma blocks of the unit's nm MCUs, at ny; phase 1: its chroma blocks, Cb and Cr interleaved, at nc, then -- where the filter runs -- the
// left neighbours' and the right neighbours' blocks of both
JS_REN_HD uint32_t js_rs_n(const JsRsRec& r, uint32_t phase) { return phase ? r.nc : r.ny; }
JS_REN_HD uint32_t js_rs_jobs(const JsRsRec& r, uint32_t nm, uint32_t phase)
{
    if (!phase) return nm * (r.ncomp == 1u ? 1u : r.H * r.V);
    return r.ncomp == 1u ? 0u : 2u * nm + (js_rs_filtered(r) ? 4u : 0u);
}
// Job jb of phase `phase` of the unit (my, m0, nm): exists -- the block is there; blk -- its arena row, relative to the image's first; keep -- 1: all n samples
// of result row k go to bytes cell0 + k * JS_RS_PITCH + (0 .. n - 1); 2: the last sample alone, 3: the first alone, to byte cell0 + k * JS_RS_PITCH.
struct JsRsJob { uint32_t exists, keep, cell0; uint64_t blk; };
JS_REN_HD JsRsJob js_rs_job(const JsRsRec& r, uint32_t my, uint32_t m0, uint32_t nm, uint32_t phase, uint32_t jb)
{
    JsRsJob j; j.exists = 0u; j.keep = 0u; j.cell0 = 0u; j.blk = 0u;
    if (jb >= js_rs_jobs(r, nm, phase)) return j;
    const uint32_t nluma = r.ncomp == 1u ? 1u : r.H * r.V;
    const uint64_t row0 = (uint64_t)my * r.mcu_xmax;
    if (!phase) {
        const uint32_t m = jb / nluma, kb = jb - m * nluma, hx = kb & (r.H - 1u), vy = kb / r.H;
        j.exists = 1u; j.keep = 1u; j.blk = (row0 + m0 + m) * r.bpm + kb; j.cell0 = vy * r.ny * JS_RS_PITCH + 8u + (m * r.H + hx) * r.ny;
        return j;
    }
    if (jb < 2u * nm) {
        const uint32_t m = jb >> 1, ci = jb & 1u;
        j.exists = 1u; j.keep = 1u; j.blk = (row0 + m0 + m) * r.bpm + nluma + ci; j.cell0 = (1u + ci) * JS_RS_PLANE_BYTES + 8u + m * r.nc;
        return j;
    }
    const uint32_t h = jb - 2u * nm, ci = h & 1u;
    if (h < 2u) { if (m0 == 0u) return j; j.keep = 2u; j.blk = (row0 + m0 - 1u) * r.bpm + nluma + ci; j.cell0 = (1u + ci) * JS_RS_PLANE_BYTES + 7u; }
    else { if (m0 + nm >= r.mcu_xmax) return j; j.keep = 3u; j.blk = (row0 + m0 + nm) * r.bpm + nluma + ci; j.cell0 = (1u + ci) * JS_RS_PLANE_BYTES + 8u + nm * r.nc; }
    j.exists = 1u;
    return j;
}

// four samples of one 4:2:2 chroma component for pixels 2 i0 .. 2 i0 + 3 of unit row ly: p = the component's plane in the wave's LDS, c0 = the plane column of
// the unit's first own sample (m0 * nc), wc = its own samples (nm * nc).  The index is clamped to the real extent dw, then made local.  Replication where libjpeg
// does not filter: denom 8, and dw <= 2 (there the second index also stays on the unit's own cells: the pixels it would serve lie past the unit).
JS_REN_HD void js_rs_chroma4(const uint8_t* p, uint32_t ly, uint32_t i0, uint32_t dw, uint32_t c0, uint32_t wc, bool filtered, uint32_t out[4])
{
    const uint8_t* row = p + ly * JS_RS_PITCH + 8u;
    if (!filtered || dw <= 2u) {
        const uint32_t last = (dw < c0 + wc ? dw : c0 + wc) - 1u;
        const uint32_t a = row[(int)((i0 > last ? last : i0) - c0)], b = row[(int)((i0 + 1u > last ? last : i0 + 1u) - c0)];
        out[0] = a; out[1] = a; out[2] = b; out[3] = b;
        return;
    }
    uint32_t s[4];
    for (int k = 0; k < 4; k++) { const int i = (int)i0 - 1 + k; const uint32_t g = i < 0 ? 0u : ((uint32_t)i >= dw ? dw - 1u : (uint32_t)i); s[k] = row[(int)g - (int)c0]; }
    uint32_t e, o;
    js_ren_h2v1(s[0], s[1], s[2], &e, &o); out[0] = e; out[1] = o;
    js_ren_h2v1(s[1], s[2], s[3], &e, &o); out[2] = e; out[3] = o;
}

// ---------------------------------------------------------------------------------------------- sizes, plan (host)
inline int js_rs_denom(unsigned denom, const char* who)
{
    if (denom != 1u && denom != 2u && denom != 4u && denom != 8u) { js_set_error("%s: denom = %u, one of 1, 2, 4, 8 is rendered", who, denom); return -1; }
    return 0;
}
inline uint32_t js_rs_out(uint32_t dim, unsigned denom) { return (dim + denom - 1u) / denom; }
inline uint32_t js_rs_run(uint32_t H, uint32_t m) { return 64u / (H * m); }
inline uint64_t js_rs_units(const JsImage& im, uint32_t H, unsigned denom) { const uint32_t run = js_rs_run(H, 8u / denom); return (uint64_t)im.mcu_ymax * ((im.mcu_xmax + run - 1u) / run); }
inline uint64_t js_rs_dense_row(const JsImage& im, const JsnoopPackSpec& s, unsigned denom) { return (uint64_t)js_rs_out(im.dim_x, denom) * js_pack_elem(s) * (s.layout == JSNOOP_PACK_HWC ? 3u : 1u); }
inline uint64_t js_rs_dense_bytes(const JsImage& im, const JsnoopPackSpec& s, unsigned denom) { return (uint64_t)js_rs_out(im.dim_x, denom) * js_rs_out(im.dim_y, denom) * 3u * js_pack_elem(s); }

// Checks every argument of one call at denom 2, 4 or 8 and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_pack_import_spec(.., "pack_ijg_scaled").  The destination checks are jsnoop_batch_pack_ijg's, against the reduced size.
inline int js_rs_plan(const JsImage* imgs, size_t nimg, const JsnoopPackSpec& s, unsigned denom, const int* images, int n, const JsnoopPackDst* dst, JsRsRec* recs, uint32_t* unit_base)
{
    if (denom != 2u && denom != 4u && denom != 8u) { js_set_error("pack_ijg_scaled: denom = %u, one of 2, 4, 8 has a plan of this kind", denom); return -1; }
    uint64_t units = 0;
    const uint32_t m = 8u / denom;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_ijg_scaled: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        uint32_t H = 1, V = 1;
        if (js_ren_renderable(im, i, &H, &V)) return -1;
        const JsnoopPackDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack_ijg_scaled: destination %d (image %d) is NULL", k, i); return -1; }
        const uint32_t ox = js_rs_out(im.dim_x, denom), oy = js_rs_out(im.dim_y, denom);
        const uint64_t dense_row = js_rs_dense_row(im, s, denom), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack_ijg_scaled: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        const uint64_t dense_plane = (uint64_t)oy * row_pitch;
        uint64_t plane_pitch = dense_plane;
        if (s.layout == JSNOOP_PACK_CHW) {
            if (d.plane_pitch) plane_pitch = d.plane_pitch;
            if (plane_pitch < dense_plane) { js_set_error("pack_ijg_scaled: plane_pitch %llu of destination %d (image %d) is below the dense plane of %llu bytes", (unsigned long long)d.plane_pitch, k, i, (unsigned long long)dense_plane); return -1; }
        }
        if (s.dtype == JSNOOP_PACK_F32 && (((uint64_t)(uintptr_t)d.ptr | row_pitch | plane_pitch) & 3u)) {
            js_set_error("pack_ijg_scaled: float32 destination %d (image %d): pointer and pitches must be multiples of 4", k, i); return -1; }
        JsRsRec& r = recs[k];
        memset(&r, 0, sizeof r);
        r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch; r.plane_pitch = plane_pitch; r.coef_off = im.coef_off;
        r.out_x = ox; r.out_y = oy; r.ncomp = im.ncomp; r.H = H; r.V = V; r.mcu_xmax = im.mcu_xmax; r.mcu_ymax = im.mcu_ymax; r.bpm = im.blk_per_mcu;
        r.m = m; r.ny = js_rs_size(m, H, V, H, V); r.nc = im.ncomp == 3u ? js_rs_size(m, H, V, 1u, 1u) : 0u;
        r.run = js_rs_run(H, m); r.runs = (im.mcu_xmax + r.run - 1u) / r.run;
        r.dwc = im.ncomp == 3u ? (im.dim_x * r.nc + H * 8u - 1u) / (H * 8u) : 0u;
        unit_base[k] = (uint32_t)units; units += js_rs_units(im, H, denom);
        if (units >= 0x7FFFFFFFull) { js_set_error("pack_ijg_scaled: more than 2^31 units of work in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}

// ---------------------------------------------------------------------------------------------- the walk of a unit, stage by stage (host and device)
// What one lane does between two wave barriers.  k_render_ijg_scaled calls these with the barriers between them; tests/cpp/render_scaled_check.cpp calls them for
// lanes 0 .. 63 in turn over a poisoned copy of a wave's LDS.  N is the phase's transform size (wave-uniform: one switch per phase).
struct JsRsUnit { uint32_t my, m0, nm; };
struct alignas(16) JsRsV4 { uint32_t x, y, z, w; };
struct alignas(8)  JsRsV2 { uint32_t x, y; };

// load: lane (b, r) of a sub-round whose first job is jb0 fetches row r of job jb0 + b -- one 16-byte arena segment, and only where pass 1 reads that row --
// widens it (index 0 of row 0 from dccum) and writes it into the load tile
template <int N>
JS_REN_HD void js_rs_load(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t jb0, uint32_t lane, const int16_t* coef, const int16_t* dccum, uint8_t* mem)
{
    const uint32_t bl = lane >> 3, r8 = lane & 7u;
    if (!js_rs_needs(N, r8)) return;
    const JsRsJob job = js_rs_job(r, u.my, u.m0, u.nm, phase, jb0 + bl);
    if (!job.exists) return;
    const uint64_t blk = r.coef_off + job.blk;
    const JsRsV4 raw = *reinterpret_cast<const JsRsV4*>(coef + blk * 64u + r8 * 8u);
    JsRsV4 lo, hi;
    lo.x = (uint32_t)(int32_t)(int16_t)raw.x; lo.y = (uint32_t)((int32_t)raw.x >> 16); lo.z = (uint32_t)(int32_t)(int16_t)raw.y; lo.w = (uint32_t)((int32_t)raw.y >> 16);
    hi.x = (uint32_t)(int32_t)(int16_t)raw.z; hi.y = (uint32_t)((int32_t)raw.z >> 16); hi.z = (uint32_t)(int32_t)(int16_t)raw.w; hi.w = (uint32_t)((int32_t)raw.w >> 16);
    if (r8 == 0u) lo.x = (uint32_t)(int32_t)dccum[blk];
    uint32_t* tb = reinterpret_cast<uint32_t*>(mem + JS_RS_OFF_TILE) + bl * JS_RS_BLK_PITCH + r8 * 8u;
    *reinterpret_cast<JsRsV4*>(tb) = lo; *reinterpret_cast<JsRsV4*>(tb + 4) = hi;
}
// pass 1: lane (b, c) reads column c of the tile of job jb0 + b (the rows the transform reads), runs the column step and writes the N results into workspace
// rows (q 8 + b) N + k, column c -- q the sub-round inside the group
template <int N>
JS_REN_HD void js_rs_pass1(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t jb0, uint32_t q, uint32_t lane, uint8_t* mem)
{
    const uint32_t bl = lane >> 3, c = lane & 7u;
    if (!js_rs_needs(N, c)) return;
    const JsRsJob job = js_rs_job(r, u.my, u.m0, u.nm, phase, jb0 + bl);
    if (!job.exists) return;
    const int32_t* tb = reinterpret_cast<const int32_t*>(mem + JS_RS_OFF_TILE) + bl * JS_RS_BLK_PITCH + c;
    int32_t d[8], o[8];
    #if defined(__HIPCC__)
    #pragma unroll
    #endif
    for (int v = 0; v < 8; v++) d[v] = js_rs_needs(N, (uint32_t)v) ? tb[v * 8] : 0;
    if (N == 8) { js_ren_idct_step<11>(d); for (int k = 0; k < 8; k++) o[k] = d[k]; }
    else if (N == 4) js_rs_step4<12>(d, o);
    else js_rs_step2<13>(d, o);
    int32_t* ws = reinterpret_cast<int32_t*>(mem + JS_RS_OFF_WS);
    #if defined(__HIPCC__)
    #pragma unroll
    #endif
    for (int k = 0; k < N; k++) ws[js_rs_ws_row((q * 8u + bl) * N + k) + c] = o[k];
}
// pass 2: lane L reads workspace row L -- row k = L % N of job g0 + L / N -- runs the row step, saturates and writes what the job keeps into the byte planes
template <int N>
JS_REN_HD void js_rs_pass2(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t g0, uint32_t lane, uint8_t* mem)
{
    const uint32_t jg = lane / N, k = lane % N;
    const JsRsJob job = js_rs_job(r, u.my, u.m0, u.nm, phase, g0 + jg);
    if (!job.exists) return;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(mem + JS_RS_OFF_WS) + js_rs_ws_row(lane);
    const JsRsV4 lo = *reinterpret_cast<const JsRsV4*>(w), hi = *reinterpret_cast<const JsRsV4*>(w + 4);
    int32_t d[8] = { (int32_t)lo.x, (int32_t)lo.y, (int32_t)lo.z, (int32_t)lo.w, (int32_t)hi.x, (int32_t)hi.y, (int32_t)hi.z, (int32_t)hi.w }, o[8];
    if (N == 8) { js_ren_idct_step<18>(d); for (int i = 0; i < 8; i++) o[i] = d[i]; }
    else if (N == 4) js_rs_step4<19>(d, o);
    else js_rs_step2<20>(d, o);
    uint32_t s[8];
    for (int i = 0; i < N; i++) s[i] = js_ren_sample(o[i]);
    uint8_t* dst = mem + job.cell0 + k * JS_RS_PITCH;
    if (job.keep == 2u) dst[0] = (uint8_t)s[N - 1];
    else if (job.keep == 3u) dst[0] = (uint8_t)s[0];
    else if (N == 8) { JsRsV2 p; p.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24); p.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24); *reinterpret_cast<JsRsV2*>(dst) = p; }
    else if (N == 4) *reinterpret_cast<uint32_t*>(dst) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    else *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(s[0] | (s[1] << 8));
}
// a phase transformed 1 x 1: lane = job; dccum alone is read, no arena byte
JS_REN_HD void js_rs_dc_job(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t jb, const int16_t* dccum, uint8_t* mem)
{
    const JsRsJob job = js_rs_job(r, u.my, u.m0, u.nm, phase, jb);
    if (job.exists) mem[job.cell0] = (uint8_t)js_ren_sample(js_rs_dc(dccum[r.coef_off + job.blk]));
}
// pixels: lane (ly4 = lane >> 4, lane & 15) makes the four pixels from x = x0 + 4 (lane & 15) of picture row y0 + ly, ly = ly0 + ly4: byte c of v[j] = output
// channel c of pixel j.  Returns how many of the four lie inside the picture (0: the lane has nothing to store), and where they go.
JS_REN_HD uint32_t js_rs_pixels(const JsRsRec& r, const JsRsUnit& u, uint32_t lane, uint32_t ly0, bool bgr, const uint8_t* mem, uint32_t* x, uint32_t* y, uint32_t v[4])
{
    const uint32_t ow = r.H * r.m, oh = r.V * r.m, x0 = u.m0 * ow, y0 = u.my * oh, lx = (lane & 15u) * 4u, ly = ly0 + (lane >> 4);
    const uint32_t wpix = u.nm * ow < r.out_x - x0 ? u.nm * ow : r.out_x - x0, hpix = oh < r.out_y - y0 ? oh : r.out_y - y0;
    if (lx >= wpix || ly >= hpix) return 0u;
    const uint32_t at = ly * JS_RS_PITCH + 8u + lx;
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(mem + at);
    if (r.ncomp == 1u) { for (int j = 0; j < 4; j++) v[j] = ((y4 >> (8 * j)) & 0xFFu) * 0x010101u; }
    else {
        uint32_t cb[4], cr[4];
        if (r.H == 2u && r.V == 1u) {
            js_rs_chroma4(mem + JS_RS_PLANE_BYTES, ly, (x0 + lx) >> 1, r.dwc, u.m0 * r.nc, u.nm * r.nc, js_rs_filtered(r), cb);
            js_rs_chroma4(mem + 2u * JS_RS_PLANE_BYTES, ly, (x0 + lx) >> 1, r.dwc, u.m0 * r.nc, u.nm * r.nc, js_rs_filtered(r), cr);
        } else {
            const uint32_t b4 = *reinterpret_cast<const uint32_t*>(mem + JS_RS_PLANE_BYTES + at), r4 = *reinterpret_cast<const uint32_t*>(mem + 2u * JS_RS_PLANE_BYTES + at);
            for (int j = 0; j < 4; j++) { cb[j] = (b4 >> (8 * j)) & 0xFFu; cr[j] = (r4 >> (8 * j)) & 0xFFu; }
        }
        for (int j = 0; j < 4; j++) {
            const uint32_t rgb = js_ren_rgb((y4 >> (8 * j)) & 0xFFu, cb[j], cr[j]);
            v[j] = bgr ? ((rgb >> 16) & 0xFFu) | (rgb & 0xFF00u) | ((rgb & 0xFFu) << 16) : rgb;
        }
    }
    *x = x0 + lx; *y = y0 + ly;
    return wpix - lx < 4u ? wpix - lx : 4u;
}
